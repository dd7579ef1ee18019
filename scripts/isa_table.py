#!/usr/bin/env python
"""Static instruction mix of the kernels of one HIP source, from its gfx950 device assembly.

    python scripts/isa_table.py [csrc/kernels/convnet_step2.hip] [--filter fwd --filter bwd]

Per kernel: VALU / SALU / branch (part of SALU) / LDS / VMEM / SMEM instruction counts and
the total, from the assembly of the build's exact compilation
(``_build.hip_kernel_cmd(..., device_asm=True)``); VGPRs, SGPR / VGPR spill counts and the
scratch size from the kernel metadata.  Counts are static (code size), not what a wave
executes: a wave branches around paths its launch does not take.  CPU only (hipcc
cross-compiles); also prints the wall time of the compilation.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

META_KEYS = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size")


def classify(mn: str) -> str:
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def kernel_metadata(text: str) -> dict:
    """{symbol: {key: int}} from the amdhsa.kernels metadata at the end of the assembly."""
    out, cur = {}, None
    inside = False
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line.startswith("amdhsa."):
            break
        # a kernel's own keys sit at indent 4 (the first behind "  - "); its arguments deeper
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        k, v = m.group(2), m.group(3).strip()
        if k in META_KEYS:
            cur[k] = int(v)
        elif k == ".symbol":
            out[v.strip("'\"").removesuffix(".kd")] = cur
    return out


def _simple_demangle(sym: str) -> str:
    """`_ZN4damd8convnet23fwdILb1EEEv...` -> `damd::convnet2::fwd<true>` (nested names and
    bool template arguments only: enough for this project's kernels)."""
    if not sym.startswith("_ZN"):
        return sym
    i, parts = 3, []
    while i < len(sym) and sym[i].isdigit():
        j = i
        while sym[j].isdigit():
            j += 1
        n = int(sym[i:j])
        parts.append(sym[j:j + n])
        i = j + n
    name = "::".join(parts)
    if sym[i:i + 1] == "I":
        args = re.findall(r"Lb([01])E", sym[i:sym.index("EE", i) + 1])
        name += "<" + ", ".join("true" if a == "1" else "false" for a in args) + ">"
    return name


def demangle(names):
    import shutil

    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if tool:
        try:
            r = subprocess.run([tool, *names], capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: _simple_demangle(n) for n in names}


def short(name: str) -> str:
    """`void damd::convnet2::fwd<true>(...)` -> `convnet2::fwd<true>`."""
    n = re.sub(r"^void\s+", "", name)
    n = n.split("(")[0]
    return n.removeprefix("damd::")


def table(src: Path, defines=()) -> tuple:
    """([(kernel, counts dict)], compile seconds): one entry per kernel of `src`."""
    import check_publish_isa as cpi
    from distributed_amd import _build

    with tempfile.TemporaryDirectory() as td:
        asm = Path(td) / (src.name + ".s")
        t0 = time.time()
        r = subprocess.run(_build.hip_kernel_cmd(src, asm, defines, device_asm=True), capture_output=True, text=True)
        dt = time.time() - t0
        if r.returncode != 0:
            raise RuntimeError(f"device assembly build failed:\n{r.stderr[-2000:]}")
        text = asm.read_text()
    meta = kernel_metadata(text)
    fns = cpi.parse_asm(text)
    names = demangle([n for n in fns if n in meta])
    rows = []
    for sym, pretty in names.items():
        c = dict(valu=0, salu=0, branch=0, lds=0, vmem=0, smem=0, other=0)
        for mn in fns[sym].mnemonics():
            k = classify(mn)
            c[k] += 1
            if mn.startswith(("s_cbranch", "s_branch")):
                c["branch"] += 1
        c["total"] = sum(v for k, v in c.items() if k != "branch")
        c.update({k.lstrip("."): v for k, v in meta[sym].items()})
        rows.append((short(pretty), c))
    return rows, dt


def render(rows) -> str:
    cols = ["valu", "salu", "branch", "lds", "vmem", "smem", "total", "vgpr_count", "sgpr_spill_count",
            "vgpr_spill_count", "private_segment_fixed_size", "kernarg_segment_size"]
    head = ["VALU", "SALU", "branch", "LDS", "VMEM", "SMEM", "total", "VGPRs", "sgpr_spill", "vgpr_spill", "scratch_B",
            "kernarg_B"]
    w = max(len(n) for n, _ in rows)
    lines = [f"{'kernel':<{w}}  " + " ".join(f"{h:>10}" for h in head)]
    for n, c in sorted(rows):
        lines.append(f"{n:<{w}}  " + " ".join(f"{c.get(k, 0):>10}" for k in cols))
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source", nargs="?", default=str(ROOT / "csrc" / "kernels" / "convnet_step2.hip"))
    ap.add_argument("--filter", action="append", default=[], help="only kernels whose name contains this")
    a = ap.parse_args(argv)
    src = Path(a.source).resolve()
    rows, dt = table(src)
    if a.filter:
        rows = [r for r in rows if any(f in r[0] for f in a.filter)]
    print(f"# {src.name}: static gfx950 instruction mix per kernel (branch is part of SALU); compiled in {dt:.1f} s")
    print(render(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
