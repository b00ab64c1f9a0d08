"""Pin the numpy oracle to the reference on a GENERAL graph (CPU only): the fixtures of
tests/golden/make_golden_graph.py (EGNO.forward and SEGNO forward_step run by the reference itself on
the 37-node test graph of tests/_graph_case.py: isolated nodes, an in-degree-40 receiver, a self loop,
a duplicate edge). The GPU tests of the general-graph kernels compare against this oracle. Bars as
tests/test_oracle_golden.py uses for its forward fixtures."""
import numpy as np
import pytest

from oracle import egno as oe
from oracle import segno as osg
from tests._graph_case import ISOLATED, HUB, HUB_DEG, egno_case, segno_case
from tests.conftest import load_golden, maxnorm_rel, params_of

TOL32 = 1e-5   # SURVEY §8d parity bound (max-norm relative, fp32)


def test_fixture_graph_is_the_seeded_test_graph():
    g = load_golden("egno_graph")
    n = int(g["cfg::n"])
    c = egno_case(load_golden("egno_fwd"), n)
    assert np.array_equal(g["in::row"], c["row"]) and np.array_equal(g["in::col"], c["col"])
    assert np.array_equal(g["in::edge_attr"], c["edge_fea"])
    deg = np.bincount(c["row"], minlength=n)
    assert all(deg[i] == 0 for i in ISOLATED) and deg[HUB] == HUB_DEG and deg[n - 1] >= 1
    pairs = list(zip(c["row"].tolist(), c["col"].tolist()))
    assert (3, 3) in pairs and pairs.count((9, 4)) >= 2
    assert n % 16 != 0 and len(pairs) == int(deg.sum()) and len(pairs) > HUB_DEG + (n - 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_egno_forward_on_general_graph(dtype):
    fx, g = load_golden("egno_fwd"), load_golden("egno_graph")
    c = egno_case(fx, int(g["cfg::n"]))
    p = {k: v.astype(dtype) for k, v in params_of(fx).items()}
    a = {k: (v.astype(dtype) if k not in ("row", "col", "t_out") else v) for k, v in c.items()}
    x, v, h = oe.egno_forward(p, **a, T=int(g["cfg::T"]))
    assert maxnorm_rel(x, g["out::x"]) < TOL32
    assert maxnorm_rel(v, g["out::v"]) < TOL32
    assert maxnorm_rel(h, g["out::h"]) < TOL32


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_segno_forward_step_on_general_graph(dtype):
    fx, g = load_golden("segno_fwd"), load_golden("segno_graph")
    c = segno_case(fx, int(g["cfg::n"]))
    assert np.array_equal(g["in::row"], c["row"]) and np.array_equal(g["in::edge_attr"], c["edge_attr"])
    p = {k: v.astype(dtype) for k, v in params_of(fx).items()}
    x, h, v = osg.forward(p, c["his"].astype(dtype), c["x"].astype(dtype), c["row"], c["col"], c["v"].astype(dtype),
                          c["edge_attr"].astype(dtype), T=int(g["cfg::T"]), bug_compat=False)
    assert maxnorm_rel(x, g["step::x"]) < TOL32
    assert maxnorm_rel(v, g["step::v"]) < TOL32
    assert maxnorm_rel(h, g["step::h"]) < TOL32
