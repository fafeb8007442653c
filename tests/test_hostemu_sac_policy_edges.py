"""SAC's policy head at its numeric edges through the C ABI on the g++ emulation build: the checks of tests/sac_edge_util.py
(clip and its gradient mask, saturated tanh, the EPS guards, sd ~ EPS, alpha = 0.2) on the host-side launch plan and the
per-element helpers the device shares.  The device code around them runs in tests/test_gpu_sac_policy_edges.py."""
import pytest

import sac_edge_util as se
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    return dict(backend=NumpyHostBackend(), lib_path=hostemu_lib)


@pytest.mark.parametrize("run", se.ELEMENT_RUNS, ids=se.run_id)
def test_elements_against_the_closed_form(emu, monkeypatch, capfd, run):
    se.run_elements(run, monkeypatch, capfd, **emu)


@pytest.mark.parametrize("run", se.END_TO_END_RUNS, ids=se.run_id)
def test_two_updates_against_the_float64_oracle(emu, monkeypatch, capfd, run):
    se.run_end_to_end(run, monkeypatch, capfd, **emu)


@pytest.mark.parametrize("run", se.ACT_RUNS, ids=se.run_id)
def test_actions_against_the_float64_oracle(emu, monkeypatch, run):
    se.run_act(run, monkeypatch, **emu)


def test_behaviour_cloning_on_saturated_columns(emu):
    se.run_behaviour_cloning(**emu)


def test_a_call_of_three_updates_equals_three_calls(emu):
    se.run_call_of_three_equals_three_calls(**emu)


def test_graph_replay_equals_eager(emu, monkeypatch):
    se.run_graph_replay_equals_eager(monkeypatch, **emu)
