"""The constant-configuration MNIST step kernels (fwd_flag / bwd_flag, convnet_step2.hip) on
the gfx950 device assembly of the build's own compilation: no register spills, no scratch,
and less code than the generic kernels they replace.  Reads kernel metadata and instruction
counts only (scripts/isa_table.py).  CPU only: hipcc cross-compiles."""
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


# (specialised kernel, the generic instantiation the same launch would otherwise run)
PAIRS = [("convnet2::fwd_flag<true>", "convnet2::fwd<true>"),
         ("convnet2::fwd_flag<false>", "convnet2::fwd<false>"),
         ("convnet2::bwd_flag<true>", "convnet2::bwd<true, true>"),
         ("convnet2::bwd_flag<false>", "convnet2::bwd<false, true>")]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("spec,generic", PAIRS)
def test_specialised_kernels_do_not_spill_and_are_smaller(kernels, spec, generic):
    assert spec in kernels and generic in kernels, sorted(kernels)
    s, g = kernels[spec], kernels[generic]
    print(spec, s)
    print(generic, g)
    assert s["sgpr_spill_count"] == 0
    assert s["vgpr_spill_count"] == 0
    assert s["private_segment_fixed_size"] == 0
    assert s["total"] > 0
    for k in ("total", "valu", "salu", "branch", "lds", "vmem"):
        assert s[k] < g[k], (k, s[k], g[k])
    assert s["kernarg_segment_size"] < g["kernarg_segment_size"]
