#!/usr/bin/env python3
"""What the batch's predecessor rows cost (measurement, not a test).

Graphs: the web-Google-shaped graph (generate_webgraph() defaults) with the MS1024 sources of
bench.py (the 1024 smallest ids with out-degree >= 1), and Kronecker s20 ef16 weighted 1..255
with 64 sampled roots.

(a) pj_sssp_batch_parents next to pj_sssp_batch on the same build: the cost of the feature.
    Both sides copy every row they produce into host arrays allocated once (the parents side
    moves twice the bytes); the device times (pj_stats.kernel_ms, pj_last_parents_ms) are
    listed beside the wall times.
(b) pj_sssp_batch_parents next to the only way to these rows without it, pj_sssp +
    pj_parent_tree per source, on a 64-source subset.
(c) unit weights: option batch_parents_path 1 (one edge scan per row) next to 2 (the level
    archive), device time of the parent rows.
The two sides of each comparison alternate inside one process; a warm-up of each comes first,
and the warm-up's rows are compared (batch rows == the loop's rows).

  python tools/batch_parents_bench.py [--repeats 7] [--out profiles/r07/batch_parents.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paralleljohnson_amd as pj  # noqa: E402


def spread(xs):
    return f"median {statistics.median(xs):10.3f}  min {min(xs):10.3f}  max {max(xs):10.3f}"


def alternate(repeats, sides):
    """sides: name -> callable returning a dict of numbers; every repeat runs all sides, the order
    alternating; the first round is the warm-up. Returns name -> key -> list."""
    names = list(sides)
    got = {k: {} for k in names}
    for i in range(repeats + 1):
        for k in (names if i % 2 else names[::-1]):
            r = sides[k]()
            if i:
                for key, x in r.items():
                    got[k].setdefault(key, []).append(x)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=int, default=20, help="Kronecker scale of the weighted graph")
    ap.add_argument("--ms-sources", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ptr(x):
        return x.ctypes.data_as(ctypes.c_void_p)

    def compare(g, sources, subset, label, unit):
        n = g.n
        src = np.ascontiguousarray(np.asarray(sources, dtype=np.int64))
        dist = np.empty((len(src), n), np.int32)
        par = np.empty((len(src), n), np.int32)
        dist[:] = 0  # (pages faulted in before anything is timed)
        par[:] = 0

        def plain():
            t0 = time.perf_counter()
            rc = pj._lib.pj_sssp_batch(g._h, ptr(src), len(src), ptr(dist))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            return {"wall": ms, "kernel": g.stats()["kernel_ms"]}

        def parents():
            t0 = time.perf_counter()
            g.sssp_batch_parents(src, out=(dist, par))
            ms = (time.perf_counter() - t0) * 1e3
            return {"wall": ms, "kernel": g.stats()["kernel_ms"], "parents": g.last_parents_ms()}

        r = alternate(a.repeats, {"plain": plain, "parents": parents})
        say()
        say(f"(a) {label}: {len(src)} sources, every row copied to the host "
            f"({4 * n * len(src) / 1e9:.2f} GB per block); ms per batch")
        say(f"  pj_sssp_batch          wall      {spread(r['plain']['wall'])}")
        say(f"  pj_sssp_batch_parents  wall      {spread(r['parents']['wall'])}")
        say(f"  pj_sssp_batch          kernel_ms {spread(r['plain']['kernel'])}")
        say(f"  pj_sssp_batch_parents  kernel_ms {spread(r['parents']['kernel'])}")
        say(f"  pj_last_parents_ms               {spread(r['parents']['parents'])}")
        say(f"  parent rows / solves (device, medians) "
            f"{statistics.median(r['parents']['parents']) / statistics.median(r['parents']['kernel']):.2f}; "
            f"wall ratio {statistics.median(r['parents']['wall']) / statistics.median(r['plain']['wall']):.2f}")

        sub = np.ascontiguousarray(np.asarray(subset, dtype=np.int64))
        sd = np.empty((len(sub), n), np.int32)
        sp = np.empty((len(sub), n), np.int32)
        ld = np.empty(n, np.int32)
        lp = np.empty((len(sub), n), np.int64)
        lp[:] = 0
        st = pj.Stats()

        def batch():
            t0 = time.perf_counter()
            g.sssp_batch_parents(sub, out=(sd, sp))
            ms = (time.perf_counter() - t0) * 1e3
            return {"wall": ms, "device": g.stats()["kernel_ms"] + g.last_parents_ms()}

        def loop():
            km = 0.0
            t0 = time.perf_counter()
            for i, s in enumerate(sub):
                assert pj._lib.pj_sssp(g._h, int(s), ptr(ld)) == 0
                km += g.stats_into(st).kernel_ms
                assert pj._lib.pj_parent_tree(g._h, ptr(lp[i])) == 0
            ms = (time.perf_counter() - t0) * 1e3
            return {"wall": ms, "solve_kernel": km}

        batch()
        loop()
        assert (sp == lp).all(), "batch parent rows differ from the loop's"
        r = alternate(a.repeats, {"batch": batch, "loop": loop})
        say(f"(b) {label}: {len(sub)} sources, ms for all of them")
        say(f"  pj_sssp_batch_parents            wall {spread(r['batch']['wall'])}")
        say(f"  pj_sssp + pj_parent_tree loop    wall {spread(r['loop']['wall'])}")
        say(f"  batch: solves + parent rows, device   {spread(r['batch']['device'])}")
        say(f"  loop: the solves' kernel_ms alone     {spread(r['loop']['solve_kernel'])}")
        say(f"  loop / batch (wall medians) {statistics.median(r['loop']['wall']) / statistics.median(r['batch']['wall']):.2f}")

        if unit:
            def path(p):
                def run():
                    g.set_option("batch_parents_path", p)
                    g.sssp_batch_parents(src, out=(dist, par))
                    return {"parents": g.last_parents_ms(), "kernel": g.stats()["kernel_ms"]}
                return run

            g.set_option("batch_parents_path", 1)
            g.sssp_batch_parents(src, out=(dist, par))
            keep = par.copy()
            g.set_option("batch_parents_path", 2)
            g.sssp_batch_parents(src, out=(dist, par))
            assert (keep == par).all(), "batch_parents_path 1 and 2 differ"
            del keep
            r = alternate(a.repeats, {"rows": path(1), "masks": path(2)})
            g.set_option("batch_parents_path", 0)
            say(f"(c) {label}: {len(src)} sources, pj_last_parents_ms per batch")
            say(f"  batch_parents_path 1 (per row)        {spread(r['rows']['parents'])}")
            say(f"  batch_parents_path 2 (level archive)  {spread(r['masks']['parents'])}")
            say(f"  the solves' kernel_ms beside them     {spread(r['masks']['kernel'])}")
            say(f"  per row / archive (medians) "
                f"{statistics.median(r['rows']['parents']) / statistics.median(r['masks']['parents']):.2f}")

    with pj.Context(0) as ctx:
        say(f"batch_parents_bench: libpj build {pj.build_id()}, {a.repeats} repeats after one warm-up, sides alternating")
        g = ctx.generate_webgraph()
        row, _, _ = g.get_csr()
        sources = np.nonzero(np.diff(row) >= 1)[0][:a.ms_sources]
        compare(g, sources, sources[:: max(1, len(sources) // 64)][:64],
                f"web-Google-shaped graph (n {g.n}, entries {g.nnz}), unit weights", True)
        g.close()
        pj.trim_device_cache()
        g = ctx.generate_kronecker(a.scale, 16, 1, weighted=True)
        roots = [int(r) for r in g.sample_roots(7, 64)]
        compare(g, roots, roots, f"Kronecker s{a.scale} ef16 weights 1..255 (n {g.n}, entries {g.nnz}), batch_streams 2", False)
        g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
