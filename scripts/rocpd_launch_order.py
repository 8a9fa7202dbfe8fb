#!/usr/bin/env python
"""Launch order of one captured MMoE step in a rocprofv3 rocpd SQLite database (`*_results.db`): the kernels between the
last two `gate_mix_fwd` launches, rotated so that the listing starts near the step's first kernel, with their device times.

    python scripts/rocpd_launch_order.py <db> > profiles/mmoe_step_launch_order.txt
"""
import sqlite3
import sys


def main(path):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name = "name" if "name" in cols else "kernel_name"
    rows = c.execute(f"select {name}, start, end from kernels order by start").fetchall()
    idx = [i for i, r in enumerate(rows) if "gate_mix_fwd" in r[0]]
    print(f"total dispatches {len(rows)}; gate_mix_fwd launches {len(idx)}")
    if len(idx) < 2:
        return
    a, b = idx[-2], idx[-1]
    print(f"launches per step: {b - a}")
    lead = 12 if a >= 12 else 0             # (the input layer's launches in front of the first gate_mix_fwd)
    for r in rows[a - lead:b - lead + 1]:
        print(f"{(r[2] - r[1]) / 1e3:9.1f} us  {r[0][:140]}")


if __name__ == "__main__":
    main(sys.argv[1])
