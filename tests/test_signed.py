"""Signed edge weights (pj_load_*_signed, potential.hip): Bellman-Ford potentials on the GPU,
negative-cycle detection, Johnson's reweighting and the back-transformed rows, against the
plain numpy reference of tests/signed_ref.py (exact: integer work)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import signed_ref as R
from conftest import ROOT

INF = 100000

CLRS = [(0, 1, 3), (0, 2, 8), (0, 4, -4), (1, 3, 1), (1, 4, 7), (2, 1, 4), (3, 0, 2), (3, 2, -5), (4, 3, 6)]
CLRS_H = [0, -1, -5, 0, -4]
CLRS_ROWS = [[0, 1, -3, 2, -4], [3, 0, -4, 1, -1], [7, 4, 0, 5, 3], [2, -1, -5, 0, -2], [8, 5, 1, 6, 0]]
NEW_SYMBOLS = ["pj_load_coo_signed", "pj_load_snap_signed", "pj_load_snap_buffer_signed", "pj_graph_potentials",
               "pj_graph_is_signed"]


def _coo(edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 3)
    return e[:, 0], e[:, 1], e[:, 2].astype(np.int32)


def _clean(rep):
    return all(v == 0 for k, v in rep.items() if k.startswith("bad_"))


# ---------------------------------------------------------------- CPU ------------

def test_header_declares_signed_api(pj):
    with open(os.path.join(ROOT, "include", "pj.h")) as f:
        text = f.read()
    assert re.search(r"PJ_ERR_NEGCYCLE\s*=\s*-10\b", text)
    assert "typedef struct pj_potential_stats" in text
    lib = ctypes.CDLL(pj.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int " + name + r"\(", text, re.M), name
        assert hasattr(lib, name) and name in pj.EXPORTS, name
    assert pj.PJError(-10, "x").name == "PJ_ERR_NEGCYCLE"
    st = pj.PotentialStats()
    assert [k for k, _ in st._fields_] == ["kernel_ms", "rounds", "relaxed_edges", "negative_edges", "cycle_checks",
                                           "cycle_vertex", "min_potential"]


def test_exports_match_header(pj):
    with open(os.path.join(ROOT, "include", "pj.h")) as f:
        names = set(re.findall(r"^\s*(?:const\s+)?[\w\s\*]+?\b(pj_\w+)\s*\(", f.read(), re.M))
    assert names == set(pj.EXPORTS) and set(NEW_SYMBOLS) <= names


def test_format_sol_prints_negative_distances(pj):
    assert pj.format_sol([-5, 0, 100000, 7]) == b"the vector is:\n-5\n0\ninf\n7\n"


def test_reference_reproduces_clrs():
    src, dst, w = _coo(CLRS)
    h, rounds = R.potentials(src, dst, w, 5)
    assert h.tolist() == CLRS_H and rounds >= 1
    assert [R.row(src, dst, w, 5, s, h).tolist() for s in range(5)] == CLRS_ROWS
    try:  # cross-check of the tiny case where scipy is installed
        import scipy.sparse as sp
        from scipy.sparse.csgraph import bellman_ford
    except ImportError:
        sp = None
    if sp is not None:
        d = bellman_ford(sp.csr_matrix((w.astype(float), (src, dst)), shape=(5, 5)), directed=True)
        assert d.astype(int).tolist() == CLRS_ROWS
    with pytest.raises(R.NegativeCycle):
        R.potentials([0, 1], [1, 0], [-3, 2], 2)
    # the contract's two caps (the cap-contract graph of the GPU test)
    src, dst, w = _coo([(0, 1, 99980), (1, 2, 0), (3, 2, -50), (2, 4, 100020)])
    h, _ = R.potentials(src, dst, w, 5)
    assert h.tolist() == [0, 0, -50, 0, 0]
    assert R.row(src, dst, w, 5, 0, h).tolist() == [0, 99980, INF, INF, INF]
    assert R.contract(R.distances(src, dst, w, 5, 2), h, 2)[1] == 1


# ---------------------------------------------------------------- GPU ------------

@pytest.mark.gpu
def test_clrs_graph(ctx, pj):
    src, dst, w = _coo(CLRS)
    g = ctx.load_coo_signed(src, dst, w)
    assert g.is_signed and g.weighted and g.n == 5 and g.nnz == 9
    h = g.potentials()
    assert h.tolist() == CLRS_H
    assert g.sssp_batch(range(5)).tolist() == CLRS_ROWS
    for s in range(5):
        assert g.sssp(s).tolist() == CLRS_ROWS[s]
        assert g.copy_dist().tolist() == CLRS_ROWS[s]
        g.sssp(s, copy=False)  # (the back-transform is made by the first reader)
        assert g.copy_dist().tolist() == CLRS_ROWS[s]
    row, col, wr = g.get_csr()
    u = np.repeat(np.arange(5), np.diff(row))
    inp = {}
    for a, b, x in CLRS:
        inp[(a, b)] = x
    assert (wr.astype(np.int64) >= 0).all()
    for a, b, x in zip(u, col, wr.astype(np.int64)):
        assert x == inp[(int(a), int(b))] + h[a] - h[b]
    d = g.sssp(0)
    par = g.parent_tree()
    assert _clean(g.validate_tree(0, par)) and par[0] == 0
    for v in range(1, 5):  # the tree is tight in the TRUE weights too
        assert d[par[v]] + inp[(int(par[v]), v)] == d[v]
    st = g.potential_stats()
    assert st["negative_edges"] == 2 and st["rounds"] >= 1 and st["cycle_vertex"] == -1 and st["min_potential"] == -5
    assert g.reach_stats()["reached"] == 5
    g.close()


@pytest.fixture(scope="module")
def random_case():
    n = 2000
    src, dst, w = R.random_signed(n)
    h, rounds = R.potentials(src, dst, w, n)
    sources = [0, 3, 411, 777, 1290, 1899, 1950, n - 1]  # (the last two are isolated)
    rows = np.stack([R.row(src, dst, w, n, s, h) for s in sources])
    rows.setflags(write=False)
    return dict(n=n, src=src, dst=dst, w=w, h=h, rounds=rounds, sources=sources, rows=rows)


@pytest.mark.gpu
def test_random_directed_graph(ctx, pj, random_case, tmp_path):
    c = random_case
    n, w = c["n"], c["w"]
    print("negative fraction", (w < 0).mean(), "h min", c["h"].min(), "jacobi rounds", c["rounds"],
          "reached from 0", int((c["rows"][0] < INF).sum()))
    # the figures of the case: a third of the weights negative, 11 Jacobi rounds, the 100 isolated ids unreached
    assert 0.32 < (w < 0).mean() < 0.34 and c["h"].min() == -49 and c["rounds"] == 11
    assert int((c["rows"][0] < INF).sum()) == 1900 and (c["rows"][0] < 0).any()
    g = ctx.load_coo_signed(c["src"], c["dst"], w, n=n)
    assert (g.potentials() == c["h"]).all()
    st = g.potential_stats()
    assert st["rounds"] >= 1 and st["negative_edges"] == int((w < 0).sum()) and st["cycle_vertex"] == -1
    assert st["min_potential"] == c["h"].min() and st["relaxed_edges"] > 0
    row, col, wr = g.get_csr()
    assert (wr == 0).any()  # (reduced weights are full of zeros)
    for i, s in enumerate(c["sources"]):
        assert (g.sssp(s) == c["rows"][i]).all(), s
        assert g.reach_stats()["reached"] == int((c["rows"][i] < INF).sum())
    par = g.parent_tree()
    assert _clean(g.validate_tree(c["sources"][-1], par))
    # in-place updates: after k rounds every h is <= Jacobi's after k rounds, so the fixpoint stands after
    # the reference's count of improving rounds; one more round runs on the last improved vertices and finds nothing
    assert 1 <= st["rounds"] <= c["rounds"] + 1
    g.set_option("delta", 3)  # options and the automatic delta work as on any weighted graph
    assert (g.sssp(0) == c["rows"][0]).all()
    g.set_option("delta", 0)
    for streams in (1, 3):
        g.set_option("batch_streams", streams)
        assert (g.sssp_batch(c["sources"]) == c["rows"]).all(), streams
        paths = [str(tmp_path / f"sol_{streams}_{i}.txt") for i in range(len(c["sources"]))]
        g.sssp_batch_write(c["sources"], paths)
        for i, p in enumerate(paths):
            assert open(p, "rb").read() == pj.format_sol(c["rows"][i]), (streams, i)
    g.close()


@pytest.mark.gpu
def test_random_graph_in_poisoned_memory(ctx):
    """The rounds enqueued past the fixpoint and every buffer of the load must hold only what this
    load wrote: a fresh child process with PJ_DEVMEM_POISON=1 (allocations start full of 0xFF)."""
    env = dict(os.environ, PJ_DEVMEM_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "signed_ref.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_wide_rows_kronecker(ctx, oracle):
    k = ctx.generate_kronecker(14, 16, 1, weighted=True)
    row, col, c = k.get_csr()
    roots = [int(r) for r in k.sample_roots(7, 4)]
    k.close()
    n = len(row) - 1
    assert np.diff(row).max() > 64  # the wave-wide row path runs
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(row))
    v = col.astype(np.int64)
    p = np.random.default_rng(7).integers(0, 101, n)
    w = (c.astype(np.int64) - p[u] + p[v]).astype(np.int32)
    assert (w < 0).any()
    h, _ = R.potentials(u, v, w, n)
    g = ctx.load_coo_signed(u, v, w, n=n)
    assert (g.potentials() == h).all()
    for s in roots:
        dc = oracle.dijkstra(row, col.astype(np.uint32), c, s).astype(np.int64)
        reach = dc < INF
        d = dc - p[s] + p
        dr = d + h[s] - h
        assert dc[reach].max() < INF - 200 and dr[reach].max() < INF and d[reach].max() < INF  # neither cap bites
        exp = np.where(reach, d, INF)
        assert (g.sssp(s) == exp).all(), s
    g.close()


@pytest.mark.gpu
def test_degenerate_shapes(ctx):
    e = np.zeros(0, np.int64)
    g = ctx.load_coo_signed(e, e, e.astype(np.int32), n=0)
    assert g.n == 0 and g.is_signed and len(g.potentials()) == 0 and len(g.sssp(0)) == 0
    assert g.sssp_batch([0, 1]).shape == (2, 0)
    g.close()
    g = ctx.load_coo_signed(e, e, e.astype(np.int32), n=1)
    assert g.potentials().tolist() == [0] and g.sssp(0).tolist() == [0] and g.sssp(1).tolist() == [INF]
    assert g.potential_stats()["rounds"] == 0
    g.close()
    g = ctx.load_coo_signed([0], [0], [5])
    assert g.n == 1 and g.potentials().tolist() == [0] and g.sssp(0).tolist() == [0]
    g.close()
    g = ctx.load_coo_signed([0, 0, 0], [1, 1, 1], [5, -2, 3])
    assert g.potentials().tolist() == [0, -2] and g.sssp(0).tolist() == [0, -2] and g.sssp(1).tolist() == [INF, 0]
    assert sorted(g.get_csr()[2].tolist()) == [0, 5, 7]
    g.close()
    g = ctx.load_coo_signed([0], [1], [-1], n=5)
    assert g.n == 5 and g.potentials().tolist() == [0, -1, 0, 0, 0]
    assert g.sssp(0).tolist() == [0, -1, INF, INF, INF]
    for s in (-1, 5, 10**12):
        assert (g.sssp(s) == INF).all()
    assert (g.sssp_batch([-1, 0, 5]) == [[INF] * 5, [0, -1, INF, INF, INF], [INF] * 5]).all()
    g.close()
    rng = np.random.default_rng(11)
    n, m = 300, 1500
    src, dst, w = rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, 40, m)
    g = ctx.load_coo_signed(src, dst, w.astype(np.int32), n=n)
    u = ctx.load_coo(src, dst, w=w.astype(np.uint32), n=n)
    st = g.potential_stats()
    assert st["rounds"] == 0 and st["negative_edges"] == 0 and st["min_potential"] == 0 and (g.potentials() == 0).all()
    assert not u.is_signed and u.potential_stats() is None
    for s in (0, 17, 299):
        assert (g.sssp(s) == u.sssp(s)).all()
    assert (g.sssp_batch([5, 6, 7]) == u.sssp_batch([5, 6, 7])).all()
    g.close()
    u.close()


@pytest.mark.gpu
def test_negative_cycles(ctx, pj):
    with pytest.raises(pj.PJError) as e:
        ctx.load_coo_signed([0], [0], [-1])
    assert e.value.name == "PJ_ERR_NEGCYCLE" and e.value.code == -10
    assert e.value.potential_stats["cycle_vertex"] == 0 and "0" in str(e.value)
    # a 3-cycle at the end of a long path: found by the predecessor check, not by n rounds
    n = 65536
    a, b, c = n - 3, n - 2, n - 1
    i = np.arange(n - 4)
    src = np.concatenate([i, [a, b, c, 10]])
    dst = np.concatenate([i + 1, [b, c, a, a]])
    w = np.concatenate([np.ones(n - 4, np.int64), [2, -4, 1, 5]]).astype(np.int32)
    with pytest.raises(pj.PJError) as e:
        ctx.load_coo_signed(src, dst, w, n=n)
    st = e.value.potential_stats
    assert e.value.name == "PJ_ERR_NEGCYCLE" and st["cycle_vertex"] in (a, b, c), st
    assert st["rounds"] < 1024 and st["cycle_checks"] >= 1 and str(st["cycle_vertex"]) in str(e.value)
    # a zero-weight cycle is no error
    g = ctx.load_coo_signed([0, 1], [1, 0], [-3, 3])
    assert g.potentials().tolist() == [0, -3]
    assert g.sssp_batch([0, 1]).tolist() == [[0, -3], [3, 0]]
    g.close()


@pytest.mark.gpu
def test_cap_contract(ctx, pj):
    src, dst, w = _coo([(0, 1, 99980), (1, 2, 0), (3, 2, -50), (2, 4, 100020)])
    g = ctx.load_coo_signed(src, dst, w)
    assert g.potentials().tolist() == [0, 0, -50, 0, 0]
    rows = {0: [0, 99980, INF, INF, INF], 3: [INF, INF, -50, 0, 99970], 2: [INF, INF, 0, INF, INF]}
    for s, exp in rows.items():
        assert g.sssp(s).tolist() == exp, s
        assert R.row(src, dst, w, 5, s).tolist() == exp
    assert g.sssp_batch([0, 3, 2]).tolist() == [rows[0], rows[3], rows[2]]
    g.sssp(2)  # vertex 4: d' = 99970 < INF <= d = 100020
    with pytest.raises(pj.PJError) as e:
        g.parent_tree()
    assert e.value.name == "PJ_ERR_RANGE"
    with pytest.raises(pj.PJError) as e:
        g.validate_tree(2, np.array([-1, -1, 2, -1, -1]))
    assert e.value.name == "PJ_ERR_RANGE"
    d = g.sssp(3)
    par = g.parent_tree()
    assert _clean(g.validate_tree(3, par))
    assert ((par == -1) == (d == INF)).all() and par.tolist() == [-1, -1, 3, 3, 2]
    g.close()


SIGNED_TEXT = b"# x\n0\t1\t-4\n1 2 +3\r\n2\t0\t2\n2 3\n"


@pytest.mark.gpu
def test_text_loaders_and_cli(ctx, pj, tmp_path):
    src, dst, w = _coo([(0, 1, -4), (1, 2, 3), (2, 0, 2), (2, 3, 0)])
    a = ctx.load_snap_buffer_signed(SIGNED_TEXT)
    b = ctx.load_coo_signed(src, dst, w)
    f = tmp_path / "g.txt"
    f.write_bytes(SIGNED_TEXT)
    c = ctx.load_snap_signed(str(f))
    h, _ = R.potentials(src, dst, w, 4)
    assert h.tolist() == [0, -4, -1, -1]
    exp = [R.row(src, dst, w, 4, s, h) for s in range(4)]
    for g in (a, b, c):
        assert g.is_signed and g.n == 4 and g.nnz == 4
        assert g.potentials().tolist() == h.tolist()
        for x, y in zip(g.get_csr(), b.get_csr()):
            assert (x == y).all()
        assert (g.sssp_batch(range(4)) == np.stack(exp)).all()
    assert a.potential_stats()["negative_edges"] == 1
    for g in (a, b, c):
        g.close()
    with pytest.raises(pj.PJError) as e:  # the unsigned grammar is unchanged
        ctx.load_snap_buffer(SIGNED_TEXT, weighted=True)
    assert e.value.name == "PJ_ERR_PARSE"
    with pytest.raises(pj.PJError) as e:  # |w| must fit int32
        ctx.load_snap_buffer_signed(b"0 1 -2147483648\n")
    assert e.value.name in ("PJ_ERR_PARSE", "PJ_ERR_RANGE")
    # the CLI
    env = dict(os.environ, PJ_SIGNED="1")
    out = tmp_path / "sol.txt"
    par = tmp_path / "par.txt"
    assert exp[0].tolist() == [0, -4, -1, -1]  # (the sol_file has negative lines)
    r = subprocess.run([pj.cli_path(), str(f), "0", str(out)], env=dict(env, PJ_PARENTS=str(par)), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "validation passed" in r.stderr, r.stderr
    assert out.read_bytes() == pj.format_sol(exp[0]) and par.read_bytes() == b"the parent tree is:\n0\n0\n1\n2\n"
    r = subprocess.run([pj.cli_path(), str(f), "0", str(tmp_path / "ms_{s}.txt")], env=dict(env, PJ_SOURCES="2,0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for s in (2, 0):
        assert (tmp_path / f"ms_{s}.txt").read_bytes() == pj.format_sol(exp[s])
    r = subprocess.run([pj.cli_path(), str(f), "0", str(out)], env=dict(env, PJ_GPUS="2"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "PJ_SIGNED" in r.stderr
    cyc = tmp_path / "cyc.txt"
    cyc.write_bytes(b"0 1 -3\n1 0 3\n1 0 -1\n")
    nosol = tmp_path / "nosol.txt"
    r = subprocess.run([pj.cli_path(), str(cyc), "0", str(nosol)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "negative-weight cycle" in r.stderr and not nosol.exists()


@pytest.mark.gpu
def test_refusals(ctx, pj, tmp_path):
    g = ctx.load_coo_signed([0, 1], [1, 2], [-1, 2])
    with pytest.raises(pj.PJError) as e:
        g.save(str(tmp_path / "g.pjcsr"))
    assert e.value.name == "PJ_ERR_ARG" and not (tmp_path / "g.pjcsr").exists()
    out = ctypes.c_void_p()
    assert pj._lib.pj_wpart_from_graph(g._h, 0, 1, ctypes.byref(out)) == -1 and not out.value
    g.close()
    u = ctx.load_coo([0, 1], [1, 2], w=np.array([1, 2], np.uint32))
    with pytest.raises(pj.PJError) as e:
        u.potentials()
    assert e.value.name == "PJ_ERR_STATE"
    u.close()
