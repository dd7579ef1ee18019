"""The two compile-time switches of the flagship kernels' decode work (convnet_step2.hip):
DAMD_FIXW (the wave-uniform 32-bit fixed-point decode) and DAMD_BWD_CGPRE (the conv gradient on
pre-decoded argmax codes).  Statically, from the kernel metadata of a gfx950 compilation
(scripts/isa_table.py): with either or both at 0 the flagship kernels still compile without
spills or scratch inside 128 VGPRs, each switch changes the code of the kernels it names and
of no other, and the default build has both on.  CPU only: hipcc cross-compiles."""
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

_FLAG = ("convnet2::fwd_flag<true>", "convnet2::fwd_flag<false>", "convnet2::bwd_flag<true>", "convnet2::bwd_flag<false>")
_MIX = ("valu", "salu", "lds", "vmem", "total")
_TABLES = {}


def _table(defines=()):
    if defines not in _TABLES:
        import isa_table

        rows, _ = isa_table.table(ROOT / "csrc" / "kernels" / "convnet_step2.hip", defines=defines)
        _TABLES[defines] = dict(rows)
    return _TABLES[defines]


def _mix(k):
    return tuple(k[m] for m in _MIX)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("defines", [("DAMD_FIXW=0",), ("DAMD_BWD_CGPRE=0",), ("DAMD_FIXW=0", "DAMD_BWD_CGPRE=0")],
                         ids=["decode-off", "convgrad-off", "both-off"])
def test_switches_off_compile_clean_and_change_only_their_kernels(defines):
    on, off = _table(), _table(defines)
    assert on.keys() == off.keys()
    for name in _FLAG:
        k = off[name]
        assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
    # the forward has only the decode; the backward has both
    fwd_changes = "DAMD_FIXW=0" in defines
    for name in on:
        changed = _mix(on[name]) != _mix(off[name])
        if "bwd_flag" in name:
            assert changed, name
        elif "fwd_flag" in name:
            assert changed == fwd_changes, name
        else:  # the generic kernels, flush, gather: neither switch reaches them
            assert not changed, name


@pytest.mark.timeout(600)
def test_default_build_has_both_on():
    assert _mix(_table()["convnet2::bwd_flag<true>"]) == _mix(_table(("DAMD_FIXW=1", "DAMD_BWD_CGPRE=1"))["convnet2::bwd_flag<true>"])
    from distributed_amd import native

    C = native.load_C()
    # the conv role's LDS holds the 2-byte entries: 4 KB more than a byte per code would take
    conv, w1 = C.convnet2_bwd_role_lds_bytes(2, 0), C.convnet2_bwd_role_lds_bytes(2, 1)
    assert conv == 146496 and w1 < conv <= 160 * 1024, (conv, w1)
