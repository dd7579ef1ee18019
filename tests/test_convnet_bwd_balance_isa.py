"""The flagship backward (bwd_flag, convnet_step2.hip) on its wave mapping, statically: from the
kernel metadata of the build's own gfx950 compilation (scripts/isa_table.py) neither
instantiation spills a register or uses scratch, and on 16 waves it stays within the 128
VGPRs a 1024-thread block may use; the LDS size the launcher asks for fits one workgroup.
CPU only: hipcc cross-compiles."""
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    import isa_table

    rows, _ = isa_table.table(ROOT / "csrc" / "kernels" / "convnet_step2.hip")
    return dict(rows)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["convnet2::bwd_flag<true>", "convnet2::bwd_flag<false>"])
def test_bwd_flag_registers(kernels, name):
    assert name in kernels, sorted(kernels)
    k = kernels[name]
    print(name, k)
    assert k["sgpr_spill_count"] == 0
    assert k["vgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    nt = k["max_flat_workgroup_size"]  # the launch bound: CfgFlagBwd::NT
    assert nt in (512, 1024)
    if nt == 1024:
        assert k["vgpr_count"] <= 128


def test_bwd_flag_lds_fits_one_workgroup():
    from distributed_amd import native

    C = native.load_C()
    flag, generic = C.convnet2_bwd_flag_lds_bytes(2), C.convnet2_lds_bytes(2)[1]
    assert generic <= flag <= 163840, (generic, flag)
