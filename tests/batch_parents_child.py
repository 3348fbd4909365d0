"""Child process of test_batch_parents.py::test_fresh_graph_in_poisoned_memory: started with
PJ_DEVMEM_POISON=1 (every device allocation starts full of 0xFF), it loads a fresh graph and its
very first call is sssp_batch_parents."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    assert os.environ.get("PJ_DEVMEM_POISON") == "1"
    import paralleljohnson_amd as pj
    from helpers import random_graph, tight_parents
    n = 4001
    rng = np.random.default_rng(21)
    src, dst = random_graph(rng, "hub", n)
    sources = rng.integers(0, n, 90)
    with pj.Context(0) as ctx:
        g = ctx.load_coo(src, dst, n=n)
        dist, par = g.sssp_batch_parents(sources)
        row, col, _ = g.get_csr()
        for i, s in enumerate(sources):
            assert (par[i] == tight_parents(row, col, None, dist[i], int(s))).all(), i
        assert (dist == g.sssp_batch(sources)).all()
        g.close()
    print("batch parents poison ok")


if __name__ == "__main__":
    main()
