#!/usr/bin/env python3
"""Compare the device code of two ``build/`` directories kernel for kernel.

Both directories come from ``python optical-flow_dexi-raft_amd/build.py --force
--asm``, which keeps one device ``.s`` per translation unit.  Kernels are keyed by
(unit stem, kernel symbol), so the same template instantiated in two units is
two kernels — unlike compare_resource_usage.py, which keys by the source file of
a kernel's definition.  For every kernel in both builds the script compares

* the instruction stream: the text between the kernel's label and its
  ``.Lfunc_end``, comments stripped, local labels renumbered by first use;
* the ``.amdhsa_kernel`` descriptor block.

It only compares text.  Kernels present on one side only are listed per unit.
Exit status 1 if any common kernel differs, or (with ``--same-set``) if the sets
differ.

Usage: compare_kernel_isa.py BASE_BUILD_DIR NEW_BUILD_DIR [--same-set] [--allow-gone SUBSTR]
"""
from __future__ import annotations

import argparse
import re
import sys
from pathlib import Path

DEVICE_SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def _normalise(lines: list[str]) -> list[str]:
    """Instruction lines without comments, local labels renumbered by first use."""
    names: dict[str, str] = {}

    def rename(m: re.Match) -> str:
        return names.setdefault(m.group(0), f".L{len(names)}")

    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if line:
            out.append(LOCAL_LABEL.sub(rename, line))
    return out


def kernels(asm: Path) -> dict[str, tuple[list[str], list[str]]]:
    """symbol -> (instruction stream, descriptor block) of every kernel in one .s file."""
    lines = asm.read_text().splitlines()
    descs: dict[str, list[str]] = {}
    for i, line in enumerate(lines):
        if line.strip().startswith(".amdhsa_kernel "):
            sym = line.split()[1]
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            descs[sym] = [l.strip() for l in lines[i:end + 1]]
    found = {}
    for i, line in enumerate(lines):
        sym = line.split(":", 1)[0]
        if line.startswith("_Z") and sym in descs and line[len(sym):].startswith(":"):
            end = next(j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end"))
            found[sym] = (_normalise(lines[i + 1:end]), descs[sym])
    missing = set(descs) - set(found)
    if missing:
        raise RuntimeError(f"{asm.name}: no body found for {sorted(missing)}")
    return found


def units(build_dir: Path) -> dict[str, dict]:
    return {p.name[:-len(DEVICE_SUFFIX)]: kernels(p) for p in sorted(build_dir.glob("*" + DEVICE_SUFFIX))}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("base", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--same-set", action="store_true", help="fail if the kernel sets differ")
    ap.add_argument("--allow-gone", action="append", default=[], metavar="SUBSTR",
                    help="with --same-set: a kernel whose symbol contains SUBSTR may be absent from NEW")
    a = ap.parse_args()
    base, new = units(a.base), units(a.new)
    bad = False
    print(f"{'unit':<24} {'base':>5} {'new':>5} {'same':>5} {'differ':>6} {'gone':>5} {'added':>5}")
    notes = []
    for u in sorted(set(base) | set(new)):
        b, n = base.get(u, {}), new.get(u, {})
        common = sorted(set(b) & set(n))
        differ = [k for k in common if b[k] != n[k]]
        gone, added = sorted(set(b) - set(n)), sorted(set(n) - set(b))
        print(f"{u:<24} {len(b):>5} {len(n):>5} {len(common) - len(differ):>5} {len(differ):>6} "
              f"{len(gone):>5} {len(added):>5}")
        for k in differ:
            what = "instructions" if b[k][0] != n[k][0] else "descriptor"
            notes.append(f"DIFFER {u}: {k} ({what})")
        notes += [f"GONE   {u}: {k}" for k in gone] + [f"ADDED  {u}: {k}" for k in added]
        bad |= bool(differ)
        if a.same_set:
            bad |= bool(added) or any(not any(s in k for s in a.allow_gone) for k in gone)
    print(f"{'total':<24} {sum(map(len, base.values())):>5} {sum(map(len, new.values())):>5}")
    print("\n".join(notes))
    print("FAIL" if bad else "OK: every common kernel has the same instructions and descriptor")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
