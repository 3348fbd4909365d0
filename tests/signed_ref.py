"""Plain numpy reference of the signed-weight path (pj_load_*_signed): int64 Bellman-Ford
with np.minimum.at for the potentials h (from h = 0 everywhere) and for single-source
distances, and the output contract of include/pj.h ("signed edge weights") applied in int64.
Shared by tests/test_signed.py; run as a script it is the child process of the poison test."""
import numpy as np

INF = 100000
BIG = np.int64(1) << 50  # "no path" inside the reference


class NegativeCycle(Exception):
    pass


def _arr(src, dst, w):
    return (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), np.asarray(w, dtype=np.int64))


def potentials(src, dst, w, n):
    """h[v] = min(0, min_u d(u, v)): Jacobi rounds from h = 0; (h, rounds that changed something)."""
    src, dst, w = _arr(src, dst, w)
    h = np.zeros(n, np.int64)
    for rounds in range(n + 1):
        new = h.copy()
        if len(src):
            np.minimum.at(new, dst, h[src] + w)
        if (new == h).all():
            return h, rounds
        h = new
    raise NegativeCycle


def distances(src, dst, w, n, s):
    """True distances from s (BIG = no path); an out-of-range source reaches nothing."""
    src, dst, w = _arr(src, dst, w)
    d = np.full(n, BIG, np.int64)
    if not 0 <= s < n:
        return d
    d[s] = 0
    for _ in range(n + 1):
        new = d.copy()
        ok = d[src] < BIG
        if ok.any():
            np.minimum.at(new, dst[ok], d[src[ok]] + w[ok])
        if (new == d).all():
            return d
        d = new
    raise NegativeCycle


def contract(d, h, s):
    """out[v] = INF if d'(s,v) >= INF, INF if d(s,v) >= INF, else d(s,v); d' = d + h[s] - h[v].
    Also returns the number of vertices with d' < INF <= d."""
    n = len(d)
    out = np.full(n, INF, np.int64)
    if not 0 <= s < n:
        return out.astype(np.int32), 0
    path = d < BIG
    dr = np.where(path, d + h[s] - h, BIG)
    keep = path & (dr < INF) & (d < INF)
    out[keep] = d[keep]
    return out.astype(np.int32), int((path & (dr < INF) & (d >= INF)).sum())


def row(src, dst, w, n, s, h=None):
    if h is None:
        h, _ = potentials(src, dst, w, n)
    return contract(distances(src, dst, w, n, s), h, s)[0]


def random_signed(n=2000, live=1900, m=16000, seed=5):
    """The random directed case of the tests: costs c in [0, 20], potentials p in [0, 50],
    w = c - p[src] + p[dst] (no negative cycle: every cycle weighs its costs); the ids from
    `live` on are isolated."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, live, m)
    dst = rng.integers(0, live, m)
    c = rng.integers(0, 21, m)
    p = rng.integers(0, 51, n)
    return src, dst, (c - p[src] + p[dst]).astype(np.int32)


def _poison_child():
    """Fresh process with PJ_DEVMEM_POISON=1 (every device allocation starts full of 0xFF): the
    signed load and solves of the random case must not depend on memory they did not write."""
    import os
    import sys
    assert os.environ.get("PJ_DEVMEM_POISON") == "1"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import paralleljohnson_amd as pj
    n = 2000
    src, dst, w = random_signed(n)
    h, _ = potentials(src, dst, w, n)
    with pj.Context(0) as ctx:
        for _ in range(2):  # (the second load takes the first one's freed blocks)
            g = ctx.load_coo_signed(src, dst, w, n=n)
            assert (g.potentials() == h).all()
            srcs = [0, n - 1, n + 3, 7]
            exp = np.stack([row(src, dst, w, n, s, h) for s in srcs])
            assert (g.sssp_batch(srcs) == exp).all()
            for i, s in enumerate(srcs):
                assert (g.sssp(s) == exp[i]).all()
            rep = g.validate_tree(srcs[-1], g.parent_tree())
            assert all(v == 0 for k, v in rep.items() if k.startswith("bad_")), rep
            g.close()
    print("poison ok")


if __name__ == "__main__":
    _poison_child()
