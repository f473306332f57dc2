// contact_rows.h -- what a contact mode (4 bits, one per foot) means for the equality-constraint set of a node and for its projection: which row is
// whose, which rows ad_node_kernel stores, which force inputs are pinned and which are free directions of Pu, and the weight-compensating nominal input.
// constexpr functions of (mode, index) only -- no device state -- so that ad_node_kernel (writes the rows), lq_node_kernel (reads them, projects), the
// consumers of the stage record (riccati_kernel, ddp_kernel, feedback_kernel: rebuild the force rows of Pu), the line search and host code agree by construction;
// the static_asserts at the end check the structure for all sixteen modes.
//
// Rows, in the insertion order of the reference (QMInterface.cpp:116-131), foot by foot:
//   stance foot: 3 zero-velocity rows;
//   swing foot:  3 zero-force rows (C = 0, D = unit vector on force input 3 leg + q, e = u: known from the mode, NOT stored by ad_node_kernel), then 1 normal-velocity row.
#pragma once
#include "layout.h"

namespace qmk {

constexpr int FEET = 4, FORCE_INPUTS = 3 * FEET;
constexpr int STANCE_ROWS = 3, ZERO_FORCE_ROWS = 3, SWING_ROWS = ZERO_FORCE_ROWS + 1;   // rows of a stance foot; zero-force rows and all rows of a swing foot

constexpr bool contactOf(int mode, int leg) { return (mode >> (3 - leg)) & 1; }
constexpr int stanceCount(int mode) {
  int n = 0;
  for (int leg = 0; leg < FEET; ++leg) n += contactOf(mode, leg) ? 1 : 0;
  return n;
}

// ---- rows of the constraint set
constexpr int rowsOfFoot(int mode, int leg) { return contactOf(mode, leg) ? STANCE_ROWS : SWING_ROWS; }
constexpr int firstRowOfFoot(int mode, int leg) {   // (leg = FEET: the number of rows)
  int row = 0;
  for (int k = 0; k < FEET; ++k) if (k < leg) row += rowsOfFoot(mode, k);
  return row;
}
constexpr int constraintCount(int mode) { return firstRowOfFoot(mode, FEET); }   // nc, 12..16
// force input that row r pins to zero (a swing foot's zero-force row), or -1 (a velocity row, or r >= nc)
constexpr int zeroForceInputOfRow(int mode, int r) {
  int row = 0, res = -1;
  for (int k = 0; k < FEET; ++k) {
    if (!contactOf(mode, k) && r >= row && r < row + ZERO_FORCE_ROWS) res = 3 * k + (r - row);
    row += rowsOfFoot(mode, k);
  }
  return res;
}
// what ad_node_kernel writes: the velocity rows; and the first of them (a stance foot's first row or a swing foot's normal-velocity row)
constexpr bool rowIsStored(int mode, int r) { return r >= 0 && r < constraintCount(mode) && zeroForceInputOfRow(mode, r) < 0; }
constexpr int firstStoredRow(int mode) { return contactOf(mode, 0) ? 0 : ZERO_FORCE_ROWS; }
// velocity rows (the rows that depend on the inputs through the joint velocities only): nv = 3 stance + swing <= 12, and the row of the r-th of them (0 for r >= nv)
constexpr int velocityRowCount(int mode) { return STANCE_ROWS * stanceCount(mode) + (FEET - stanceCount(mode)); }
constexpr int rowOfVelocityRow(int mode, int r) {
  int nv = 0, res = 0;
  for (int k = 0; k < FEET; ++k) {
    const int n = contactOf(mode, k) ? STANCE_ROWS : 1, first = firstRowOfFoot(mode, k) + (contactOf(mode, k) ? 0 : ZERO_FORCE_ROWS);
    if (r >= nv && r < nv + n) res = first + (r - nv);
    nv += n;
  }
  return res;
}

// ---- force inputs i < 12 (foot i / 3, axis i % 3): pinned by a row (swing foot) or a free direction of the projection (stance foot)
constexpr int pinningRowOfForce(int mode, int i) { return contactOf(mode, i / 3) ? -1 : firstRowOfFoot(mode, i / 3) + i % 3; }   // or -1: free
constexpr int freeForceCount(int mode) { return 3 * stanceCount(mode); }
// column of Pu that carries the unit entry of force input i < 12, or -1 (swing foot): stance feet in foot order, three columns each
constexpr int puColumnOfForce(int mode, int i) {
  int nb = 0, col = -1;
  for (int leg = 0; leg < FEET; ++leg) { const int st = contactOf(mode, leg); if (st && i / 3 == leg) col = 3 * nb + i % 3; nb += st; }
  return col;
}

// ---- nominal input (QMInitializer.cpp:33-41, the tracking cost's u_nominal): the weight shared by the stance feet on their z entries, nothing else
template <class T> constexpr T nominalNormalForce(T mass, T gravity, int mode) {
  const int nStance = stanceCount(mode);
  return nStance > 0 ? mass * gravity / nStance : T(0);
}
template <class T> constexpr T nominalInputEntry(int mode, int i, T fzNom) { return (i < FORCE_INPUTS && (i % 3) == 2 && contactOf(mode, i / 3)) ? fzNom : T(0); }

// ---- the structure, checked for every mode
template <class Pred> constexpr bool everyMode(Pred holds) {
  for (int mode = 0; mode < 16; ++mode) if (!holds(mode)) return false;
  return true;
}
constexpr bool rowCountsHold(int mode) {
  const int st = stanceCount(mode), sw = FEET - st, nc = constraintCount(mode), nv = velocityRowCount(mode), mt = NU - nc;
  return nc == 3 * st + 4 * sw && nc <= NCMAX && mt >= 14 && mt <= MT && nv + ZERO_FORCE_ROWS * sw == nc && nv <= 12 && freeForceCount(mode) + (18 - nv) == mt;
}
constexpr bool rowsPartition(int mode) {   // the velocity rows, in order, are exactly the rows of the set that pin no force, and exactly the stored rows
  int nvSeen = 0;
  for (int r = 0; r < NCMAX; ++r) {
    const bool zf = zeroForceInputOfRow(mode, r) >= 0, inSet = r < constraintCount(mode), vel = nvSeen < velocityRowCount(mode) && rowOfVelocityRow(mode, nvSeen) == r;
    if ((inSet ? zf == vel : (zf || vel)) || vel != rowIsStored(mode, r)) return false;
    nvSeen += vel ? 1 : 0;
  }
  return nvSeen == velocityRowCount(mode) && rowIsStored(mode, firstStoredRow(mode));
}
constexpr bool pinningIsInverse(int mode) {
  for (int i = 0; i < FORCE_INPUTS; ++i) { const int r = pinningRowOfForce(mode, i); if (r >= 0 && zeroForceInputOfRow(mode, r) != i) return false; }
  for (int r = 0; r < NCMAX; ++r) { const int i = zeroForceInputOfRow(mode, r); if (i >= 0 && pinningRowOfForce(mode, i) != r) return false; }
  return true;
}
constexpr bool freeForcesFillPu(int mode) {
  int next = 0;
  for (int i = 0; i < FORCE_INPUTS; ++i) { const int col = puColumnOfForce(mode, i); if ((col >= 0) != (pinningRowOfForce(mode, i) < 0) || (col >= 0 && col != next++)) return false; }
  return next == freeForceCount(mode);
}
static_assert(everyMode(rowCountsHold), "nc = 3 stance + 4 swing <= NCMAX, m~ = 30 - nc in [14, MT], nv + 3 swing = nc, free forces + (18 - nv) = m~");
static_assert(everyMode(rowsPartition), "every row is exactly one of zero-force or velocity; the velocity rows are the stored ones; firstStoredRow is stored");
static_assert(everyMode(pinningIsInverse), "pinningRowOfForce and zeroForceInputOfRow are inverse to each other");
static_assert(everyMode(freeForcesFillPu), "a force input has a Pu column exactly when no row pins it, and those columns are 0 .. freeForceCount - 1 in foot order");

}  // namespace qmk
