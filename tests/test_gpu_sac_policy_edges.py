"""SAC's policy head at its numeric edges on the MI355X (tests/sac_edge_util.py has the regimes, the float64 references and
every bound): the log-std clip and its gradient mask, saturated tanh, the EPS guards, sd ~ EPS and alpha = 0.2 through

  training  mlp (96, 72), obs 29, A = 7, B = 17 (two 16-row blocks, the second ragged; ragged A): the VALU chains (the default at
            this width, and under GRL_NO_HEADS_MFMA) and, under GRL_NO_FUSED_HEADS, a launch per layer with sample_kernel,
            sample_bwd_kernel and sac_loss_kernel; mlp (48, 40) at the same B and A: heads_fused_kernel on the matrix cores; mlp
            (260,), B = 5, A = 5: wider than HT_MAXW, per layer without a switch; the augmented depth extractor, B = 6 (the staged
            CNN plan); mlp (64, 64) at B = 1.  Each handle's route is read from its GRL_PLAN_DUMP.
  acting    act_heads_mfma_kernel, act_heads_kernel (GRL_TUNE act_mfma=0) and act_out_kernel, calls of 1 and 17 rows
  behaviour cloning on saturated columns, and the bits: one call of three updates against three calls, graph replay against eager."""
import pytest

import sac_edge_util as se

pytestmark = pytest.mark.gpu


def test_the_runs_cover_the_three_head_routes():
    assert {se.ROUTE[(shape, switch)] for shape, switch, _ in se.ELEMENT_RUNS} == {"one_launch", "chains", "per_layer"}
    assert {se.ROUTE[(shape, switch)] for shape, switch, _ in se.END_TO_END_RUNS} == {"one_launch", "chains", "per_layer"}


@pytest.mark.parametrize("run", se.ELEMENT_RUNS, ids=se.run_id)
def test_elements_against_the_closed_form(monkeypatch, capfd, run):
    se.run_elements(run, monkeypatch, capfd)


@pytest.mark.parametrize("run", se.END_TO_END_RUNS, ids=se.run_id)
def test_two_updates_against_the_float64_oracle(monkeypatch, capfd, run):
    se.run_end_to_end(run, monkeypatch, capfd)


@pytest.mark.parametrize("run", se.ACT_RUNS, ids=se.run_id)
def test_actions_against_the_float64_oracle(monkeypatch, run):
    se.run_act(run, monkeypatch)


def test_behaviour_cloning_on_saturated_columns():
    se.run_behaviour_cloning()


def test_a_call_of_three_updates_equals_three_calls():
    se.run_call_of_three_equals_three_calls()


def test_graph_replay_equals_eager(monkeypatch):
    se.run_graph_replay_equals_eager(monkeypatch)
