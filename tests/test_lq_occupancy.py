"""lq_node_kernel runs three wavefronts per SIMD: its kernel descriptor must leave room for twelve single-wave workgroups
per CU, in LDS and in the unified register file, without scratch.  Read from the device assembly of both builds that ship the kernel (fp64 `lq`,
fp32 `mpc32`), compiled exactly as the library compiles them.  The bound is checked on the descriptor itself, not on the compiler's occupancy
remark, which rounds the LDS-limited workgroup count up to whole wavefronts per SIMD."""
import os
import re
import shutil
import tempfile

import pytest

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 12          # one wavefront each: three per SIMD
VGPRS_PER_WAVE = 168            # 512 unified VGPR + AGPR per lane / 3, in granules of 8


def _kernel_metadata(text, symbol):
    meta = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - ", meta):
        fields = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)", entry, re.M))
        if fields.get("name") == symbol:
            return fields
    raise AssertionError(f"no kernel descriptor for {symbol}")


@pytest.mark.parametrize("unit,symbol", [("lq", "_ZN3qmk14lq_node_kernelENS_6LqArgsE"), ("mpc32", "_ZN5qmk3214lq_node_kernelENS_6LqArgsE")])
def test_lq_node_kernel_fits_three_wavefronts_per_simd(unit, symbol):
    from qm_door_amd import build as qb
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm, = qb.device_asm(tmp, units=[unit])
        md = _kernel_metadata(open(asm).read(), symbol)
    lds, vgpr, agpr, scratch = (int(md[k]) for k in ("group_segment_fixed_size", "vgpr_count", "agpr_count", "private_segment_fixed_size"))
    assert WORKGROUPS_PER_CU * lds <= LDS_PER_CU, f"{unit}: {lds} B of LDS per workgroup"
    assert vgpr <= VGPRS_PER_WAVE, f"{unit}: {vgpr} registers (VGPR + AGPR)"
    assert agpr <= vgpr, f"{unit}: {agpr} AGPRs outside the unified count {vgpr}"
    assert scratch == 0, f"{unit}: {scratch} B of scratch per lane"
