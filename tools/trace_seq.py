#!/usr/bin/env python3
"""per-launch table of the vocoder convolution family from a rocprofv3 rocpd database: the launches of one forward in stream order,
durations averaged over the last `iters` forwards.  usage: trace_seq.py results.db n_forwards iters"""
import sqlite3, sys, re
if len(sys.argv) != 4:
    sys.exit(__doc__)
db, nf, iters = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
c = sqlite3.connect(db)
cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
st = "start" if "start" in cols else ("start_time" if "start_time" in cols else None)
if st is None:
    print("columns:", cols); sys.exit(1)
rows = c.execute(f"select name, grid_x, grid_y, lds_size, vgpr_count, duration from kernels where name like '%dtts%' and (name like '%rb2x_kernel%' or name like '%rblock_kernel%' or name like '%vpair_kernel%' or name like '%vconv_kernel%') order by {st}").fetchall()
n = len(rows)
if n % nf:
    print(f"{n} launches do not divide into {nf} forwards"); nf = 1
per = n // nf
print(f"{n} launches, {per} per forward; averages over the last {iters} forwards")
print("| # | kernel | grid | lds | vgpr | avg us | min us |")
print("|---|---|---|---|---|---|---|")
tot = 0
for i in range(per):
    ds = [rows[f * per + i][5] for f in range(nf - iters, nf)]
    name = rows[(nf - 1) * per + i][0]
    m = re.search(r"(\w+_kernel<[^>]*>)", name)
    r = rows[(nf - 1) * per + i]
    tot += sum(ds) / len(ds)
    print(f"| {i} | `{m.group(1) if m else name[:60]}` | {r[1]}x{r[2]} | {r[3]} | {r[4]} | {sum(ds) / len(ds) / 1e3:.1f} | {min(ds) / 1e3:.1f} |")
print(f"\nsum {tot / 1e6:.3f} ms per forward")
