"""The f16x3 node stage and edge kernel are compiled for three waves per SIMD (168 registers on gfx950), which they fit
only with spills — and every spill has to sit behind the range vote, in the bf16x6 fallback body that in-range data
never executes.  This compiles the matrix-core translation unit's device code (`make -C groupnet_amd/csrc spills`, no
GPU needed) and checks the listing with tools/spill_regions.py."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "groupnet_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {"node_stage_kernel<2,float>": "node_stage_kernelILi2EfEE", "edge_x_kernel<2,float>": "edge_x_kernelILi2EfEE"}

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spills"))
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    run = subprocess.run(["make", "-C", CSRC, "spills", f"HIPCC={hipcc}", f"SPILLS_DIR={out}", "SPILLS_ARGS=--json"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    rep = json.loads(run.stdout[run.stdout.index("{"):run.stdout.rindex("}") + 1])
    sys.stdout.write("\n" + json.dumps({k: v for k, v in rep.items() if any(m in k for m in KERNELS.values())}, indent=1))
    return rep


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_three_wave_kernels_keep_their_spills_behind_the_vote(report, kernel):
    found = [r for name, r in report.items() if KERNELS[kernel] in name]
    assert len(found) == 1, (kernel, list(report))
    r = found[0]
    assert r["fp16_mfma"] > 0 and r["bf16_mfma"] > 0            # both bodies are there and can be told apart
    assert r["vgprs"] <= 168, r                                  # three waves per SIMD: 512 / 3, in granules of 8
    assert r["occupancy"] >= 3, r
    assert r["inside"] == 0, r                                   # no scratch among the fp16 MFMAs
    # no scratch on any path that reaches the kernel's end without a bf16 MFMA (prologue, pooling, affinity tail,
    # epilogue): before the fp16 span, and anywhere else
    assert r["hot_before"] == 0 and r["hot"] == 0, r


def test_listing_analysis_tells_hot_from_cold():
    """The analysis itself, on a hand-written listing: one spill in the fp16 body, one behind the vote."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import spill_regions
    finally:
        sys.path.pop(0)
    body = """
	s_load_dword s0, s[4:5], 0x0
	scratch_store_dword off, v1, off
	v_mfma_f32_32x32x16_f16 v[0:15], v[16:19], v[20:23], v[0:15]
	s_cbranch_scc0 .LBB0_2
	scratch_load_dword v1, off, off
	s_endpgm
.LBB0_2:
	scratch_store_dword off, v2, off offset:4
	v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], v[20:23], v[0:15]
	s_branch .LBB0_3
.LBB0_3:
	scratch_load_dword v2, off, off offset:4
	s_endpgm
""".splitlines()
    r = spill_regions.analyse(body)
    assert (r["before"], r["inside"], r["behind"]) == (1, 0, 3)
    assert r["hot"] == 2 and r["hot_before"] == 1               # the store in the prologue and the reload of the fp16 exit
