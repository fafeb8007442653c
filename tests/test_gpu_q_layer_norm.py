"""Layer-normalised DQN / BDQ on the MI355X through the C ABI: ln_relu_fwd / ln_relu_bwd (csrc/ln_kernels.h) inside the
per-layer launch plan of csrc/plan_q.inl, against the float64 restatement of tests/q_layer_norm_util.py at the shapes of
tests/test_hostemu_q_layer_norm.py -- one element per lane, tail lanes and tail rows, eight elements per lane, no trunk -- with
the route asserted from the plan dump."""
import numpy as np
import pytest

import q_layer_norm_util as lu
import q_parity_util as qu

pytestmark = pytest.mark.gpu

LN_LINE = "grl plan: q layer_norm   per-layer launches + ln_relu_fwd/bwd"


def assert_route(plan):
    assert LN_LINE in plan, plan
    assert "grl plan: q chains" not in plan and "inside the backward chains" not in plan and "grl plan: q_pf " not in plan
    assert "sampler on the apply launch): yes" not in plan
    assert "+ select kernel" in plan and "act: one launch" not in plan


@pytest.mark.parametrize("name", list(lu.LN_CASES))
def test_update_matches_the_float64_reference(name, monkeypatch, capfd):
    """forward, every gradient tensor (gamma / beta included), one optimiser step on identical inputs, three updates, target copy"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    lu.run_and_compare_ln(lu.make_ln_case(name))
    out = capfd.readouterr()
    print(out.out)
    assert_route(out.err)


@pytest.mark.parametrize("n", qu.ACT_NS)
@pytest.mark.parametrize("name", ["dqn_100_65", "bdq_shipped"])
def test_act_bins_equal_the_argmax_of_the_reference(name, n):
    lu.act_check(lu.make_ln_case(name), n)


@pytest.mark.parametrize("name", ["dqn_48", "bdq_shipped"])
def test_graph_replay_equals_eager(name, monkeypatch):
    def run(eager):
        if eager:
            monkeypatch.setenv("GRL_NO_GRAPH", "1")
        eng = lu.engine_setup(lu.make_ln_case(name, n_replay=300))
        eng.train_device(3)
        out = (eng.get_parameters(), eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy(), eng.metrics())
        eng.close()
        if eager:
            monkeypatch.delenv("GRL_NO_GRAPH")
        return out
    a, b = run(False), run(True)
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("prioritised", [False, True])
@pytest.mark.parametrize("name", ["dqn_100_65", "bdq_no_trunk"])
def test_multi_update_call_equals_single_calls(name, prioritised, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    lu.multi_update_check(name, prioritised)
    assert_route(capfd.readouterr().err)
