#!/usr/bin/env python3
"""Compare two ``-Rpass-analysis=kernel-resource-usage`` logs (``build.py --asm``
writes the remarks to stderr), kernel for kernel.

    python optical-flow_dexi-raft_amd/build.py --asm 2> parent.log   # on the parent commit
    python optical-flow_dexi-raft_amd/build.py --asm 2> new.log
    python scripts/compare_resource_usage.py parent.log new.log [--md]

Kernels are keyed by (source file, mangled name).  A trailing defaulted template
argument that a change adds (``alt_volume_gemm_kernel<T, DMA, XA>`` became
``<T, DMA, XA, float>``) changes the mangled name; ``--alias REGEX=REPL`` rewrites
the old log's mangled names (``re.sub``) before matching.  Exit status 1 when a
kernel of the first log is missing from the second or differs in any figure.
"""
from __future__ import annotations

import argparse
import re
import sys

REMARK = re.compile(r"^remark: (\S+?):\d+:\d+:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]$")
FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")


def parse(path: str) -> dict:
    out, cur = {}, None
    for line in open(path):
        m = REMARK.match(line.rstrip("\n"))
        if not m:
            continue
        src, body = m.group(1).rsplit("/", 1)[-1], m.group(2)
        if body.startswith("Function Name: "):
            cur = out.setdefault((src, body[len("Function Name: "):]), {})
        elif cur is not None and ": " in body:
            k, v = body.split(": ", 1)
            cur[k.strip()] = v.strip()
    return out


def keyed(log: dict, aliases: list[tuple[str, str]]) -> dict:
    out = {}
    for (src, name), figures in log.items():
        for old, new in aliases:
            name = re.sub(old, new, name)
        out[(src, name)] = figures
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--alias", action="append", default=[], help="OLD=NEW on the old log's names")
    ap.add_argument("--md", action="store_true", help="print the new kernels as a markdown table")
    a = ap.parse_args()
    aliases = [tuple(x.split("=", 1)) for x in a.alias]
    old, new = keyed(parse(a.old), aliases), keyed(parse(a.new), [])
    missing = [k for k in old if k not in new]
    differ = [k for k in old if k in new and any(old[k].get(f) != new[k].get(f) for f in FIELDS)]
    added = [k for k in new if k not in old]
    print(f"kernels: {len(old)} in {a.old}, {len(new)} in {a.new}; "
          f"{len(old) - len(missing) - len(differ)} identical, {len(differ)} differ, "
          f"{len(missing)} missing, {len(added)} new")
    for k in missing:
        print("MISSING", *k)
    for k in differ:
        print("DIFFERS", *k)
        for f in FIELDS:
            if old[k].get(f) != new[k].get(f):
                print(f"    {f}: {old[k].get(f)} -> {new[k].get(f)}")
    if a.md:
        print("\n| file | kernel | VGPRs | AGPRs | SGPRs | scratch | LDS | occupancy |")
        print("|---|---|---|---|---|---|---|---|")
        for k in sorted(added):
            r = new[k]
            print(f"| {k[0]} | `{k[1]}` | " + " | ".join(r.get(f, "?") for f in FIELDS[:6]) + " |")
    return 1 if missing or differ else 0


if __name__ == "__main__":
    sys.exit(main())
