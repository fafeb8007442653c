"""DQN / BDQ update and epsilon-greedy act on the MI355X at the shapes where csrc/plan_q.inl and csrc/q_act.h change kernels BY
SHAPE (tests/q_parity_util.py: SHAPE_CASES -- both sides of every such decision), against the oracle with the tolerances of the
reference shapes, and with the route each case exists for asserted from the plan dump: moving a threshold fails here instead of
silently moving a case off the kernel it covers."""
import os

import pytest

import q_parity_util as qu

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLAGS = ("chains", "mfma", "l0", "chained", "apply", "q_pf", "act")


def show(route):
    return " ".join(f if f in route else "-" for f in FLAGS)


@pytest.mark.parametrize("name", list(qu.SHAPE_CASES))
def test_update_matches_oracle_at_shape_boundaries(name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.run_and_compare(qu.make_q_case(**qu.case_args(name)))
    took = qu.route_from_dump(capfd.readouterr().err)
    print("%s: route %s" % (name, show(took)))
    assert took == qu.declared_route(name), "%s took [%s], exists for [%s]" % (name, show(took), show(qu.declared_route(name)))


def test_update_continues_the_shipped_bdq_model(monkeypatch, capfd):
    """Three updates of trained_models/BDQ_33pads_big from its shipped weights, its two real feature vectors in every minibatch:
    per-layer GEMMs at K = 512 and the three-launch apply over a 131072-float variable, against the oracle."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.run_and_compare(qu.shipped_big_trained_case(GOLD))
    assert qu.route_from_dump(capfd.readouterr().err) == qu.declared_route("shipped_big") == frozenset()


@pytest.mark.parametrize("name,n_store", [("valu_w128", 300), ("shipped_big", 300), ("B1040", 1100)])
def test_uniform_multi_update_call_off_the_matrix_core_path(name, n_store, monkeypatch, capfd):
    """One call of n uniform-replay updates == n calls of one, bit for bit, where the sequence is not the one the reference shapes
    get: q_pf around the VALU chains (valu_w128), and the plain loop where q_pf is refused by shape (no fused apply: shipped_big;
    more than 1024 rows: B1040)."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.uniform_multi_update_check(monkeypatch, name, n_store)
    plan = capfd.readouterr().err
    assert ("grl plan: q_pf " in plan) == ("q_pf" in qu.declared_route(name))


def test_per_multi_update_call_where_per_pf_is_refused_by_shape(monkeypatch, capfd):
    """obs129: no chained backward (129 observation values), so no per_pf -- one prioritised call of n updates still == n calls."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.per_multi_update_check(monkeypatch, "obs129", 3000, 2500)
    plan = capfd.readouterr().err
    assert "sampler on the apply launch): no" in plan and "sampler on the apply launch): yes" not in plan


@pytest.mark.parametrize("n", qu.ACT_NS)
@pytest.mark.parametrize("name", list(qu.SHAPE_CASES))
def test_act_bins_at_shape_boundaries(name, n, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.act_bins_check(name, n, lambda: capfd.readouterr().err)


@pytest.mark.parametrize("name", ["B_ref_ragged", "D7", "odd_widths", "obs129", "D8", "shipped_big"])
def test_all_nan_branch_gives_bin_zero(name, monkeypatch, capfd):
    """three cases on the one-launch kernel, three on the select kernel"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.nan_branch_check(name, lambda: capfd.readouterr().err)


@pytest.mark.parametrize("name", ["depth_0_4", "depth_0_3_1", "depth_2_1_2", "depth_2_2_1", "D7"])
def test_act_value_chain_reads_its_own_activations(name, monkeypatch, capfd):
    """q_parity_util.value_chain_check: value towers of two to four layers, with and without a trunk, deeper and shallower than
    the branch towers -- the hand-over from the trunk (li == Lc) and the value tower's own ping-pong buffers (li > Lc)"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qu.value_chain_check(name, lambda: capfd.readouterr().err)
