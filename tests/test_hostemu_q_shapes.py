"""The boundary shapes of tests/q_parity_util.py (SHAPE_CASES) on the CPU through the TEST-ONLY emulation build: tables,
descriptors, routing and bookkeeping of every shape against the oracle, and the table's declared routes against both a
restatement of the routing conditions and the plan the engine reports.  The emulation runs sequential reference loops in place
of the kernels and always the VALU form of the forward chains: the kernels themselves are tests/test_gpu_q_shapes.py's."""
import os

import pytest

import q_parity_util as qu
from hostemu_backend import NumpyHostBackend

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMU_FLAGS = frozenset(("chains", "chained", "apply", "q_pf", "act"))       # what the emulation build's plan can show


def test_declared_routes_follow_the_routing_conditions():
    for name in qu.SHAPE_CASES:
        assert qu.planned_route(qu.case_args(name)) == qu.declared_route(name), name


def test_every_decision_has_a_case_on_each_side():
    """no flag of the route is the same for all cases, and each one flips between two cases that the other flags allow"""
    routes = {n: qu.declared_route(n) for n in qu.SHAPE_CASES}
    for flag in ("chains", "mfma", "l0", "chained", "apply", "q_pf", "act"):
        on = [n for n, r in routes.items() if flag in r]
        assert on and len(on) < len(routes), flag
    # the pairs that sit on the two sides of ONE threshold
    for flag, yes, no in (("chains", "valu_w128", "gemm_w130"), ("chains", "valu_w128", "gemm_trunk_end_65"),
                          ("chains", "depth_3_1", "depth_3_2"), ("chains", "bins64_D5", "bins65"),
                          ("mfma", "depth_2_2_1", "valu_w65"), ("mfma", "D7", "D8"), ("l0", "obs128", "obs129"),
                          ("chained", "bins64_D4", "bins64_D5"), ("chained", "obs128", "obs129"),
                          ("apply", "qapply_edge", "qapply_over"), ("apply", "gemm_trunk_end_128", "shipped_big"),
                          ("q_pf", "B1", "B1040"), ("act", "obs128", "obs129"), ("act", "D7", "D8"),
                          ("act", "bins64_D5", "bins65"), ("act", "depth_3_1", "depth_3_2")):
        assert flag in routes[yes] and flag not in routes[no], (flag, yes, no)


@pytest.mark.parametrize("name", list(qu.SHAPE_CASES))
def test_q_plan_matches_oracle_at_shape_boundaries(hostemu_lib, name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.run_and_compare(qu.make_q_case(**qu.case_args(name)), backend=NumpyHostBackend(), lib_path=hostemu_lib)
    plan = capfd.readouterr().err
    assert "matrix-core stages" not in plan
    assert qu.route_from_dump(plan, matrix_cores=False) == qu.declared_route(name) & EMU_FLAGS, plan


def test_q_plan_continues_the_shipped_bdq_model(hostemu_lib):
    qu.run_and_compare(qu.shipped_big_trained_case(GOLD), backend=NumpyHostBackend(), lib_path=hostemu_lib)


@pytest.mark.parametrize("name,n_store", [("valu_w128", 300), ("B1040", 1100)])
def test_multi_update_uniform_call_at_shape_boundaries(hostemu_lib, name, n_store, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.uniform_multi_update_check(monkeypatch, name, n_store, backend=NumpyHostBackend(), lib_path=hostemu_lib, n=5)
    assert ("grl plan: q_pf " in capfd.readouterr().err) == ("q_pf" in qu.declared_route(name))


def test_multi_update_per_call_where_per_pf_is_refused_by_shape(hostemu_lib, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.per_multi_update_check(monkeypatch, "obs129", 2100, 2050, backend=NumpyHostBackend(), lib_path=hostemu_lib, n=6)
    plan = capfd.readouterr().err
    assert "sampler on the apply launch): no" in plan and "sampler on the apply launch): yes" not in plan


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("name", list(qu.SHAPE_CASES))
def test_act_route_and_bins_at_shape_boundaries(hostemu_lib, name, n, monkeypatch, capfd):
    """the host side of grl_act(GRL_ACT_GREEDY) -- staging, the two launch lists, the override table -- on the route of each case"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.act_bins_check(name, n, lambda: capfd.readouterr().err, backend=NumpyHostBackend(), lib_path=hostemu_lib)


@pytest.mark.parametrize("name", ["D7", "D8"])
def test_all_nan_branch_gives_bin_zero(hostemu_lib, name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.nan_branch_check(name, lambda: capfd.readouterr().err, backend=NumpyHostBackend(), lib_path=hostemu_lib)


@pytest.mark.parametrize("name", ["depth_0_4", "depth_0_3_1", "depth_2_1_2", "depth_2_2_1", "D7"])
def test_act_value_chain_reads_its_own_activations(hostemu_lib, name, monkeypatch, capfd):
    """q_parity_util.value_chain_check: value towers of two to four layers, with and without a trunk, deeper and shallower than
    the branch towers -- the hand-over from the trunk (li == Lc) and the value tower's own ping-pong buffers (li > Lc)"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.value_chain_check(name, lambda: capfd.readouterr().err, backend=NumpyHostBackend(), lib_path=hostemu_lib)
