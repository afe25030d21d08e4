"""The case tables of the f32 walk filters' CPU generators (--dump of
tests/cpp/slab_prop.cpp and tests/cpp/filter_prop.cpp, what
tests/test_walk_filters_gpu.py feeds the device): the dumped inputs, exact
verdicts and host results reproduce the counts of the plain run for the same n
and seed, and a plain run is not changed by dumping."""
import numpy as np
import pytest

import walk_tables as wt

N = 200000


@pytest.fixture(scope="module")
def gens(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_tables")
    return {k: wt.build(k, d) for k in ("slab", "filter")}, str(d)


@pytest.mark.parametrize("seed", [2025, 7])
def test_slab_table_reproduces_the_plain_run(gens, seed):
    exes, d = gens
    plain, _ = wt.run(exes["slab"], N, seed)
    dumped, t = wt.run(exes["slab"], N, seed, dump=d + "/slab.bin")
    assert dumped == plain
    n, hits, fhits, bad = plain
    assert n == N and 0 < len(t) <= N
    assert wt.slab_counts(t) == (hits, fhits, bad)
    # the inputs are what the f32 code got: the box, t_min and c hold f32 values
    f = t[:, 6:14]
    assert (f.astype(np.float32).astype(np.float64) == f).all()
    assert set(np.unique(t[:, 14])) <= {0.0, 1.0}  # skipped cases (-1) are not dumped
    # the new direction components are there: -0.0, f32-subnormal, zero in f32
    dcomp = t[:, 3:6]
    assert (np.signbit(dcomp) & (dcomp == 0)).any()
    assert (np.abs(dcomp) == 1e-40).any() and (np.abs(dcomp) == 1e-300).any()


@pytest.mark.parametrize("seed", [2025, 7])
def test_filter_table_reproduces_the_plain_run(gens, seed):
    exes, d = gens
    plain, _ = wt.run(exes["filter"], N, seed)
    dumped, t = wt.run(exes["filter"], N, seed, dump=d + "/filter.bin")
    assert dumped == plain
    n, rejected, lowered, bad = plain
    assert n == N == len(t)
    rej, low, viol = wt.filter_verdict(t, t[:, 13], t[:, 14])
    assert (rej, low, int(viol.sum())) == (rejected, lowered, bad)
    f = t[:, 6:12]
    assert (f.astype(np.float32).astype(np.float64) == f).all()
    dcomp = t[:, 3:6]
    assert (np.signbit(dcomp) & (dcomp == 0)).any()
    assert (np.abs(dcomp) == 1e-40).any() and (np.abs(dcomp) == 1e-300).any()
