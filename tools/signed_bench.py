#!/usr/bin/env python3
"""What Johnson's first phase costs (measurement, not a test).

Input: the CSR of pj_generate_kronecker(scale, 16, seed, weighted) as costs c (1..255), seeded
potentials p[v] in [0, 100], signed weights w = c - p[u] + p[v] (the graph is symmetric, so
w(u,v) + w(v,u) = 2c > 0: no negative cycle).

(a) the signed load (pj_load_coo_signed: potentials + reweighting + the usual build) next to
    pj_load_coo of the same edges with w = c (the path without the first phase);
(b) a 64-source weighted batch on the signed graph (rows copied out, so every row takes the
    back-transform pass) next to the same batch on the SAME reduced weights loaded through
    pj_load_coo: the same solver on the same rows, the difference is the pass.
The two sides of each comparison alternate inside one process; a warm-up of each comes first.

  python tools/signed_bench.py [--scale 20] [--repeats 7] [--out profiles/r07/signed_johnson.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paralleljohnson_amd as pj  # noqa: E402

INF = pj.INT_INF


def spread(xs):
    return f"median {statistics.median(xs):9.3f}  min {min(xs):9.3f}  max {max(xs):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with pj.Context(0) as ctx:
        k = ctx.generate_kronecker(a.scale, 16, a.seed, weighted=True)
        row, col, c = k.get_csr()
        roots = [int(r) for r in k.sample_roots(7, a.sources)]
        k.close()
        n, m = len(row) - 1, len(col)
        u = np.repeat(np.arange(n, dtype=np.int64), np.diff(row))
        v = col.astype(np.int64)
        p = np.random.default_rng(a.seed).integers(0, 101, n)
        w = (c.astype(np.int64) - p[u] + p[v]).astype(np.int32)
        say(f"signed_bench: libpj build {pj.build_id()}, Kronecker s{a.scale} ef16 seed {a.seed}: n {n}, entries {m}, "
            f"{(w < 0).mean() * 100:.1f}% of the weights negative, {a.repeats} repeats after one warm-up, sides alternating")

        # ---- (a) the load
        t_s, t_u, k_ms, st = [], [], [], None
        for i in range(a.repeats + 1):
            ms = {}
            for side in (("s", "u") if i % 2 else ("u", "s")):  # (the order alternates too)
                t0 = time.perf_counter()
                g = ctx.load_coo_signed(u, v, w, n=n) if side == "s" else ctx.load_coo(u, v, w=c, n=n)
                ms[side] = (time.perf_counter() - t0) * 1e3
                if side == "s":
                    st = g.potential_stats()
                g.close()
            if i:
                t_s.append(ms["s"])
                t_u.append(ms["u"])
                k_ms.append(st["kernel_ms"])
        say()
        say("(a) load, host wall ms (host id checks and H2D copies included on both sides)")
        say(f"  pj_load_coo_signed       {spread(t_s)}")
        say(f"  pj_load_coo (w = c)      {spread(t_u)}")
        say(f"  difference of medians    {statistics.median(t_s) - statistics.median(t_u):9.3f} ms  (Johnson's first phase)")
        say(f"  potentials: rounds {st['rounds']}, cycle checks {st['cycle_checks']}, relaxed edge records "
            f"{st['relaxed_edges']}, min potential {st['min_potential']}")
        say(f"  kernel_ms (rounds + reweighting, device events)  {spread(k_ms)}")
        say(f"  relaxed edge records per second (median kernel_ms): "
            f"{st['relaxed_edges'] / (statistics.median(k_ms) * 1e-3) / 1e9:.2f} G/s")

        # ---- (b) the batch
        gs = ctx.load_coo_signed(u, v, w, n=n)
        h = gs.potentials().astype(np.int64)
        rrow, rcol, rw = gs.get_csr()
        ru = np.repeat(np.arange(n, dtype=np.int64), np.diff(rrow))
        gu = ctx.load_coo(ru, rcol.astype(np.int64), w=rw, n=n)  # the same rows, no potentials
        for x, y in zip(gu.get_csr(), (rrow, rcol, rw)):
            assert (x == y).all()
        b_s, b_u, k_s, k_u = [], [], [], []
        for i in range(a.repeats + 1):
            ms, km, rows = {}, {}, {}
            for side, g in ((("s", gs), ("u", gu)) if i % 2 else (("u", gu), ("s", gs))):
                t0 = time.perf_counter()
                rows[side] = g.sssp_batch(roots)
                ms[side] = (time.perf_counter() - t0) * 1e3
                km[side] = g.stats()["kernel_ms"]
            ds, du, ks, ku = rows["s"], rows["u"], km["s"], km["u"]
            if i == 0:  # results at the size timed: every signed row is the back-transform of the reduced row
                for j, s in enumerate(roots[:8]):
                    dr = du[j].astype(np.int64)
                    d = dr - h[s] + h
                    assert (ds[j] == np.where((dr < INF) & (d < INF), d, INF)).all(), s
            else:
                b_s.append(ms["s"])
                b_u.append(ms["u"])
                k_s.append(ks)
                k_u.append(ku)
        say()
        say(f"(b) pj_sssp_batch of {len(roots)} sources, rows copied to the host, batch_streams 2; ms per batch")
        say(f"  signed graph    wall {spread(b_s)}")
        say(f"  reduced weights wall {spread(b_u)}")
        say(f"  signed graph    solver kernel_ms (sum over solves) {spread(k_s)}")
        say(f"  reduced weights solver kernel_ms (sum over solves) {spread(k_u)}")
        dm = statistics.median(b_s) - statistics.median(b_u)
        say(f"  difference of wall medians {dm:9.3f} ms = {dm / len(roots) * 1e3:.1f} us per row; the pass reads 8n and "
            f"writes 4n bytes per row ({12 * n / 1e6:.1f} MB)")
        say(f"  run-to-run spread of the unsigned side (max - min) {max(b_u) - min(b_u):.3f} ms")
        gs.close()
        gu.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
