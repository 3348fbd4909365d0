"""Predecessor rows of the batch paths (pj_sssp_batch_parents, pj_sssp_batch_write_parents,
pj_last_parents_ms): every row against helpers.tight_parents, the CPU restatement of the tree
definition, on the graph's own CSR and the batch's own distance rows (which are asserted equal to
sssp_batch), and against sssp + parent_tree per source. Unit weights run both batch_parents_path
values: 1 = one edge scan per row (tree.hip), 2 = the level archive (msbfs.hip ms_parents_k)."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import signed_ref as R
from conftest import ROOT
from helpers import random_graph, tight_parents, to_text

INF = 100000


def expected_rows(g, dist, sources):
    row, col, w = g.get_csr()
    return np.stack([tight_parents(row, col, w, dist[i], int(s)) for i, s in enumerate(sources)]).astype(np.int32)


def both_paths(g, sources):
    """(dist, parents) of the batch, after asserting that the per-row path and the archive path give
    the same blocks and that the distance rows are sssp_batch's."""
    ref = g.sssp_batch(sources)
    out = {}
    for path in (1, 2):
        g.set_option("batch_parents_path", path)
        d, p = g.sssp_batch_parents(sources)
        assert d.dtype == np.int32 and p.dtype == np.int32 and p.shape == (len(sources), g.n)
        assert (d == ref).all(), path
        out[path] = p
    g.set_option("batch_parents_path", 0)
    assert (out[1] == out[2]).all()
    return ref, out[2]


def mixed_sources(rng, n, count):
    s = rng.integers(0, n, count)
    s[5] = s[4]  # duplicates, inside one pass and across passes
    s[-1] = s[0]
    s[7] = -1  # out of range: rows of INF / -1
    s[70] = n
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("uniform", 3001), ("hub", 5003), ("chain", 1001)])
def test_random_graphs_both_paths(ctx, kind, n):
    rng = np.random.default_rng(11)
    src, dst = random_graph(rng, kind, n)
    g = ctx.load_coo(src, dst, n=n)
    assert not g.symmetric
    if kind == "hub":  # in-rows well past MS_SERIAL + 64 entries: the wave-wide walk
        assert np.bincount(dst, minlength=n).max() > 200
    g.set_option("ms_width", 1)  # 131 sources: three passes, the last of 3 sources (a partial mask word)
    sources = mixed_sources(rng, n, 131)
    dist, par = both_paths(g, sources)
    assert (par == expected_rows(g, dist, sources)).all()
    assert (par[7] == -1).all() and (par[70] == -1).all() and (par[5] == par[4]).all()
    g.close()


@pytest.mark.gpu
def test_default_width_two_words(ctx):
    n = 4099
    rng = np.random.default_rng(12)
    src, dst = random_graph(rng, "hub", n)
    g = ctx.load_coo(src, dst, n=n)
    sources = rng.integers(0, n, 70)  # W = 2, the second word holds 6 sources
    dist, par = both_paths(g, sources)
    assert (par == expected_rows(g, dist, sources)).all()
    g.close()


@pytest.mark.gpu
def test_deep_pass_falls_back(ctx):
    """More levels than archive entries (32): the pass leaves archive mode half way, and path 2
    must take the per-row path instead of reading entries that no longer hold their level."""
    n = 200
    rng = np.random.default_rng(13)
    src, dst = random_graph(rng, "chain", n)
    g = ctx.load_coo(src, dst, n=n)
    sources = [0, 1, 50, 199, 0, 120]
    g.set_option("batch_parents_path", 2)
    dist, par = g.sssp_batch_parents(sources)
    assert (dist == g.sssp_batch(sources)).all() and dist[0].max() > 40 and g.stats()["levels"] > 32
    assert (par == expected_rows(g, dist, sources)).all()
    g.close()


@pytest.mark.gpu
def test_symmetric_graph_file_order_rows(ctx):
    """Kronecker rows are out-rows in generation order: "smallest" must not depend on the row order
    (path 2 reads an id-sorted copy of the rows, path 1 the rows as they are)."""
    g = ctx.generate_kronecker(11, 16, 2)
    assert g.symmetric
    row, col, _ = g.get_csr()
    assert any((np.diff(col[row[v]:row[v + 1]]) < 0).any() for v in range(g.n))  # (the rows do not ascend)
    sources = g.sample_roots(3, 100)
    dist, par = both_paths(g, sources)
    assert (par == expected_rows(g, dist, sources)).all()
    g.close()


@pytest.mark.gpu
def test_in_rows_of_directed_graphs_ascend(ctx, tmp_path):
    """ms_parents_k takes the first hit of an in-row as the smallest tight in-neighbour: the CSC of a
    graph that is not symmetric is a stable sort of the row-major CSR by column, so its in-rows
    ascend. Checked on the host (the CSR's transpose) and on the device's own CSC, read back
    from the CSR cache file (64-byte header, row, col, crow, ccol)."""
    n = 2003
    rng = np.random.default_rng(14)
    src, dst = random_graph(rng, "hub", n)
    g = ctx.load_coo(src, dst, n=n)
    row, col, _ = g.get_csr()
    u = np.repeat(np.arange(n), np.diff(row))
    order = np.argsort(col, kind="stable")
    host_ccol, host_key = u[order], col[order]
    assert ((np.diff(host_ccol) >= 0) | (np.diff(host_key) > 0)).all()
    f = tmp_path / "g.pjcsr"
    g.save(str(f))
    raw = f.read_bytes()
    flags, = struct.unpack_from("<I", raw, 12)
    assert flags == 8  # unit weights, not symmetric, 32-bit offsets, CSC present
    nnz = g.nnz
    off = 64 + 4 * (n + 1) + 4 * nnz
    crow = np.frombuffer(raw, np.uint32, n + 1, off)
    ccol = np.frombuffer(raw, np.uint32, nnz, off + 4 * (n + 1))
    assert (crow == np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])).all()
    assert (ccol == host_ccol).all()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "hub"])
@pytest.mark.parametrize("wmax", [30, 3])
def test_weighted(ctx, kind, wmax):
    n = 5001
    rng = np.random.default_rng(15 + wmax)
    src, dst = random_graph(rng, kind, n)
    w = rng.integers(1, 31, len(src)) if wmax == 30 else rng.integers(0, 4, len(src))  # (0: the zero-weight hop rule)
    g = ctx.load_coo(src, dst, w, n=n)
    sources = [int(x) for x in rng.integers(0, n, 7)] + [-1, n]
    sources[3] = sources[0]
    single = []
    for s in sources:
        g.sssp(s)
        single.append(g.parent_tree())
    single = np.stack(single)
    for streams in (1, 3):
        g.set_option("batch_streams", streams)
        dist, par = g.sssp_batch_parents(sources)
        assert (dist == g.sssp_batch(sources)).all()
        assert (par == expected_rows(g, dist, sources)).all(), streams
        assert (par == single).all(), streams
    if wmax == 3:
        row, col, ww = g.get_csr()
        assert (ww == 0).any()
    g.close()


@pytest.mark.gpu
def test_signed_rows(ctx):
    n = 2000
    src, dst, w = R.random_signed(n)
    g = ctx.load_coo_signed(src, dst, w, n=n)
    sources = [0, 3, 411, 777, 1290, 1899, 1950, n - 1, n + 2]
    single = []
    for s in sources:
        g.sssp(s)
        single.append(g.parent_tree())
    dist, par = g.sssp_batch_parents(sources)
    assert (dist == g.sssp_batch(sources)).all() and (dist < 0).any()
    assert (par == np.stack(single)).all()
    assert ((par == -1) == (dist == INF)).all()
    g.close()


@pytest.mark.gpu
def test_signed_cap_hazard_is_refused(ctx, pj):
    """A vertex reached on the reduced weights (d' = 99,995) whose true distance is 100,005 >= INF,
    with a successor: it would be a parent of a vertex reported unreached, so the call is
    PJ_ERR_RANGE, as pj_parent_tree is. d' = d + h[s] - h[v], so the -10 sits on the source
    (h[1] = -10 through 0 -> 1) and the vertex's potential is 0."""
    src, dst, w = [0, 1, 2], [1, 2, 3], [-10, 100005, 1]
    g = ctx.load_coo_signed(src, dst, w)
    assert g.potentials().tolist() == [0, -10, 0, 0]
    assert g.sssp_batch([1, 2]).tolist() == [[INF, 0, INF, INF], [INF, INF, 0, 1]]
    with pytest.raises(pj.PJError) as e:
        g.sssp_batch_parents([2, 1])
    assert e.value.name == "PJ_ERR_RANGE" and "source 1" in str(e.value)
    g.sssp(1)
    with pytest.raises(pj.PJError) as e:  # the single-source call it mirrors
        g.parent_tree()
    assert e.value.name == "PJ_ERR_RANGE"
    dist, par = g.sssp_batch_parents([2, 0])  # rows without the hazard are served
    assert dist.tolist() == [[INF, INF, 0, 1], [0, -10, 99995, 99996]]
    assert par.tolist() == [[-1, -1, 2, 2], [0, 0, 1, 2]]
    g.close()


def _small_graph(ctx):
    n = 1203
    rng = np.random.default_rng(16)
    src, dst = random_graph(rng, "uniform", n)
    return src, dst, n


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_writer_files(ctx, pj, tmp_path, weighted):
    src, dst, n = _small_graph(ctx)
    w = np.random.default_rng(17).integers(0, 5, len(src)) if weighted else None
    g = ctx.load_coo(src, dst, w, n=n)
    sources = [2, 0, 2, n, 77]
    sol = [str(tmp_path / f"sol_{i}.txt") for i in range(len(sources))]
    par = [str(tmp_path / f"par_{i}.txt") for i in range(len(sources))]
    plain = [str(tmp_path / f"plain_{i}.txt") for i in range(len(sources))]
    g.sssp_batch_write(sources, sol, parent_paths=par)
    assert g.last_parents_ms() > 0
    g.sssp_batch_write(sources, plain)
    assert g.last_parents_ms() == 0
    for i, s in enumerate(sources):
        d = g.sssp(s)
        ref = tmp_path / "ref.txt"
        pj.write_parents(g.parent_tree(), str(ref))
        assert open(par[i], "rb").read() == ref.read_bytes(), i
        assert open(sol[i], "rb").read() == pj.format_sol(d) == open(plain[i], "rb").read(), i
    g.close()


@pytest.mark.gpu
def test_cli_batch_parents(ctx, pj, tmp_path):
    src, dst, n = _small_graph(ctx)
    web = tmp_path / "web.txt"
    web.write_bytes(to_text(src, dst))
    g = ctx.load_snap(str(web))
    env = dict(os.environ, PJ_SOURCES="2,0,2", PJ_PARENTS=str(tmp_path / "par_{i}.txt"))
    for k in ("PJ_GPUS", "PJ_WEIGHTED", "PJ_SIGNED", "PJ_CSR_CACHE"):
        env.pop(k, None)
    r = subprocess.run([pj.cli_path(), str(web), "0", str(tmp_path / "sol_{i}.txt")], env=env, capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert b"not validated on the device" in r.stderr
    for i, s in enumerate((2, 0, 2)):
        d = g.sssp(s)
        ref = tmp_path / "ref.txt"
        pj.write_parents(g.parent_tree(), str(ref))
        assert (tmp_path / f"par_{i}.txt").read_bytes() == ref.read_bytes()
        assert (tmp_path / f"sol_{i}.txt").read_bytes() == pj.format_sol(d)
    r = subprocess.run([pj.cli_path(), str(web), "0", str(tmp_path / "x_{i}.txt")],
                       env=dict(env, PJ_SOURCES="2,0", PJ_PARENTS=str(tmp_path / "same.txt")), capture_output=True,
                       timeout=120)
    assert r.returncode == 255 and b"PJ_PARENTS" in r.stderr and not (tmp_path / "same.txt").exists()
    r = subprocess.run([pj.cli_path(), str(web), "0", str(tmp_path / "y_{i}.txt")], env=dict(env, PJ_GPUS="2"),
                       capture_output=True, timeout=120)
    assert r.returncode == 255 and b"PJ_PARENTS" in r.stderr
    g.close()


@pytest.mark.gpu
def test_state_and_arguments(ctx, pj):
    src, dst, n = _small_graph(ctx)
    g = ctx.load_coo(src, dst, n=n)
    sources = np.array([5, 9, 5], np.int64)
    g.sssp(5)
    g.parent_tree()
    dist, par = g.sssp_batch_parents(sources)
    for call in (g.parent_tree, g.copy_dist):
        with pytest.raises(pj.PJError) as e:
            call()
        assert e.value.name == "PJ_ERR_STATE"
    assert g.stats()["kernel_ms"] > 0
    assert g.last_parents_ms() > 0
    assert (g.sssp_batch(sources) == dist).all()
    assert g.last_parents_ms() == 0
    only = np.empty((3, n), np.int32)  # parent_out = NULL: pj_sssp_batch
    rc = pj._lib.pj_sssp_batch_parents(g._h, sources.ctypes.data_as(ctypes.c_void_p), 3,
                                       only.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == 0 and (only == dist).all() and g.last_parents_ms() == 0
    ponly = np.empty((3, n), np.int32)  # dist_out = NULL
    rc = pj._lib.pj_sssp_batch_parents(g._h, sources.ctypes.data_as(ctypes.c_void_p), 3, None,
                                       ponly.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and (ponly == par).all()
    d0, p0 = g.sssp_batch_parents([])
    assert d0.shape == (0, n) and p0.shape == (0, n)
    with pytest.raises(pj.PJError):
        g.set_option("batch_parents_path", 3)
    g.close()


@pytest.mark.gpu
def test_fresh_graph_in_poisoned_memory(ctx):
    """The first batch of a graph launches 16 levels, well past the end of the pass, and its slots are
    fresh allocations: a fresh process with PJ_DEVMEM_POISON=1 (they start full of 0xFF) whose very
    first call is sssp_batch_parents must read only archive rows the pass wrote."""
    env = dict(os.environ, PJ_DEVMEM_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "batch_parents_child.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "batch parents poison ok" in r.stdout, r.stderr[-2000:]


def test_null_graph_is_an_argument_error(pj):
    """No device needed: the argument checks come first."""
    src = (ctypes.c_int64 * 1)(0)
    out = ctypes.c_double(-1.0)
    assert pj._lib.pj_sssp_batch_parents(None, src, 1, None, None) == -1
    assert b"pj_sssp_batch_parents" in pj._lib.pj_last_error()
    assert pj._lib.pj_sssp_batch_write_parents(None, src, 1, None, None, 0) == -1
    assert pj._lib.pj_last_parents_ms(None, ctypes.byref(out)) == -1
    assert out.value == -1.0
