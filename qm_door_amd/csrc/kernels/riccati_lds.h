// riccati_lds.h -- the dynamic LDS of one riccati_kernel workgroup: every region once, in address order (extent = rows x row stride), the overlays of
// the forward sweep and the guests of the symmetrisation scratch, each with the assertion that the guest fits its host.  The unit is `real`: the fp32 build
// carves floats with the same numbers.  riccati_kernel.h takes every offset from here.
#pragma once
#include "layout.h"
#include "real.h"
#include "lds_region.h"

namespace qmk {

// Row strides (reals) = 16 mod 32: the four k-rows x sixteen consecutive columns one MFMA operand read touches hit distinct banks
constexpr int LDS_S = 50, LDS_Y = 80, LDS_W = 48, LDS_TS = 34, LDS_LL = 18;   // LDS_LL / LDS_S: sixteen lanes one row apart (144 / 400 B) hit distinct banks: column walks are as conflict free as row walks
constexpr int STG_B = OFF_TAIL + 4;                  // reals of a record the backward sweep needs (padded)
constexpr int STG_F = STAGE_DOUBLES + GAIN_DOUBLES;  // record + gains of one stage for the forward sweep
constexpr int W_ROWS = 20, L_ROWS = 20;              // rows of W and of L: MT of data, the rest spare
constexpr int W_REALS = W_ROWS * LDS_W;              // W [20][LDS_W] of one stage
constexpr int LT_REALS = L_ROWS * LDS_LL;            // L [20][LDS_LL] row major, lower triangle; the diagonal slot holds L_cc out of the factorisation and 1 / L_cc from the stage's P6b on (riccatiInvertDiagonal)
constexpr int FWD_ZV = 80;                           // z = [dx (30) | du~ (MT) | Px dx + Pu du~ of the joint rows (30, entries 12..29 used) | 2] of one stage

// ---- the carve, in address order
using RiccatiRegion = LdsRegion<real, real>;
constexpr RiccatiRegion RL_STG{0, 2 * STG_B};                          // staging pair of the backward sweep [2][STG_B], by stage parity
constexpr auto RL_Y = ldsAfter<real>(RL_STG, 32 * LDS_Y);              // Y [32][LDS_Y]
constexpr auto RL_T = ldsAfter<real>(RL_Y, 32 * LDS_Y);                // T [32][LDS_Y]
constexpr auto RL_S = ldsAfter<real>(RL_T, 32 * LDS_S);                // S [32][LDS_S]
constexpr auto RL_W = ldsAfter<real>(RL_S, 2 * W_REALS);               // W [2][20][LDS_W] of the stage in flight and of the previous one (by stage parity): the gains of stage k + 1 are
constexpr auto RL_LT = ldsAfter<real>(RL_W, 2 * LT_REALS);             // L [2][20][LDS_LL]                  formed while stage k factorises, from W / L^T of stage k + 1
constexpr auto RL_KST = ldsAfter<real>(RL_LT, 2 * GAIN_DOUBLES);       // the gains record [2][GAIN_DOUBLES] of two stages: formed here by one wavefront, copied to HBM by two others a stage later
constexpr auto RL_SYM = ldsAfter<real>(RL_KST, 32 * LDS_TS);           // [32][LDS_TS] scratch of the wavefront-local symmetrisation (T is being read by the factorisation at that time)
constexpr auto RL_Y2 = ldsAfter<real>(RL_SYM, 16 * LDS_Y);             // [16][LDS_Y] second half of the k sum of Y rows 16..31 when only three column tiles exist (P1)
constexpr auto RL_ARMIJO = ldsAfter<real>(RL_Y2, 64);                  // the Armijo line [64]: partial slopes of the forward sweep's final reduction
constexpr int RICCATI_LDS_REALS = RL_ARMIJO.end();
constexpr int RICCATI_LDS_BYTES = RICCATI_LDS_REALS * int(sizeof(real));   // 155,904 B = 152.25 KiB at fp64, half of it at fp32 (dynamic LDS)
static_assert(RICCATI_LDS_REALS == 19488 && RICCATI_LDS_BYTES == (sizeof(real) == 8 ? 155904 : 77952), "the carve as it was measured");
static_assert(RICCATI_LDS_REALS <= 20480, "one CU's LDS at fp64");
static_assert(RL_KST.off % 2 == 0 && GAIN_DOUBLES % 2 == 0, "16-byte copies");

// ---- what the prologue's zero fills rely on: one loop each over neighbours
constexpr RiccatiRegion RL_FILL_WLK{RL_W.off, RL_W.count + RL_LT.count + RL_KST.count};   // W, L, gains images of both parities
constexpr RiccatiRegion RL_FILL_YT{RL_Y.off, RL_Y.count + RL_T.count};                    // Y, T
static_assert(RL_LT.off == RL_W.end() && RL_KST.off == RL_LT.end() && RL_FILL_WLK.end() == RL_KST.end(), "W, L and the gains images are neighbours");
static_assert(RL_T.off == RL_Y.end() && RL_FILL_YT.end() == RL_T.end(), "Y and T are neighbours");

// ---- the spare rows of L: lanes of the factorising wavefront that own no column stream their (meaningless) rows into one word of a row nobody reads
constexpr int L_SINK_ROW = L_ROWS - 1;
static_assert(MT <= L_SINK_ROW && L_SINK_ROW < L_ROWS && MT <= W_ROWS, "the idle lanes' word lies in L, behind its MT rows of data");

// ---- overlays of the forward sweep: a ring of three staging buffers [3][STG_F], then the B-operand images z of dx and du~ [3][FWD_ZV].
// Hosts: the staging pair, Y, T and S of the backward sweep, last read before the final barrier of stage 0.  The guests are first written by the forward
// prologue, behind the __syncthreads() that follows the gains epilogue: that epilogue (riccatiGains of stage 0, riccatiGainsOut) still works on W, L and the
// gains images, which is why the guests must end below RL_W -- and so below the gains images and the Armijo line, which the forward sweep keeps.
constexpr RiccatiRegion RO_RING{RL_STG.off, 3 * STG_F};
constexpr auto RO_ZV = ldsAfter<real>(RO_RING, 3 * FWD_ZV);
static_assert(RO_RING.end() <= RL_S.off && RO_ZV.end() <= RL_S.end(), "the forward ring lies over the staging pair, Y and T; the z images over the tail of T and the head of S");
static_assert(RO_ZV.end() <= RL_W.off && RO_ZV.end() <= RL_KST.off && RO_ZV.end() <= RL_ARMIJO.off, "the forward overlays stay below W, L, the gains images and the Armijo line");

// ---- guests of the symmetrisation scratch.  The wavefront-local symmetrisation (P3 phase, wavefronts 1 and 3) uses the diagonal squares (0,0) and (1,1)
// of SYM only, and only between the stage's second and third barrier.
// The parked P6a tile (0,1): rows 0..15, columns 16..31 -- a square the symmetrisation never touches.  Written by wavefront 3 in the P2 phase (three column
// tiles), read by wavefront 2 in the P3 phase.
constexpr int SYM_PARK = 16;   // first column of the parked tile
static_assert(15 * LDS_TS + SYM_PARK + 16 <= RL_SYM.count && SYM_PARK + 16 <= LDS_TS, "the parked tile's square lies inside SYM");
// The sinks of P6b (the padding entries of a tile and of its mirror image go to a word per lane): two lines of 64 at the head of SYM, written between the
// stage's third and fourth barrier, when the symmetrisation is over and the parked tile has been picked up; the next stage writes SYM behind its first barrier.
constexpr int SYM_SINK = 0, SYM_SINK_MIRROR = 64;
static_assert(SYM_SINK + 64 <= SYM_SINK_MIRROR && SYM_SINK_MIRROR + 64 <= RL_SYM.count, "the two sink lines of P6b lie inside SYM");

}  // namespace qmk
