"""SAC CnnPolicy on square images other than 64x64 on the MI355X: the per-layer implicit-GEMM route (igemm2.h / igemm_sk.h /
igemm.h over the tables of the handle's geometry), the heads, the act path on both head kernels -- against the oracle's own
arithmetic (tests/sac_image_size_util.py; tolerances of tests/parity_util.py, no ReLU hints).

hw    o1 / o2 / o3   what it can break
36     8 /  3 /  1   the minimum: dense K = 64, one output pixel
50    11 /  4 /  2   borders that no window of conv1 / conv2 covers; row counts that are no multiple of 16
84    20 /  9 /  7   the customary Nature-CNN size, K = 3136
128   31 / 14 / 12   the maximum: K = 9216, the largest tables
"""
import numpy as np
import pytest

import parity_util as pu
import sac_image_size_util as su

pytestmark = pytest.mark.gpu

NOTE = "grl plan: sac image %dx%d per-layer convolutions (conv_stack is 64x64 only)"


@pytest.mark.parametrize("name", list(su.PARITY))
@pytest.mark.parametrize("hw", [36, 50, 84])
def test_update_and_act_match_the_oracle(monkeypatch, capfd, hw, name):
    case = su.case(hw, name, 8, n_steps=4, act_batch=17)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    eng = su.parity_check(case, n_more=3)
    dump = capfd.readouterr().err
    monkeypatch.delenv("GRL_PLAN_DUMP")
    assert NOTE % (hw, hw) in dump and "conv_stack_fwd" not in dump and "conv_stack_bwd" not in dump
    su.act_check(eng, case, (1, 17))
    eng.close()


@pytest.mark.parametrize("name", list(su.PARITY))
@pytest.mark.parametrize("hw", [36, 50, 84])
def test_a_call_of_three_updates_equals_three_calls(hw, name):
    case = su.case(hw, name, 8, n_steps=1)
    out = []
    for split in ([3], [1, 1, 1]):
        eng = pu.engine_setup(case)
        for n in split:
            eng.train(n)
        out.append(su.state_of(eng) + [eng.fetch("idx_raw").copy()])
        eng.close()
    assert su.same_state(*out)


@pytest.mark.parametrize("hw", [36, 84])
def test_optimiser_step_on_identical_inputs(hw):
    pu.check_optimiser_steps(su.case(hw, n_steps=2), n=2)


def test_the_maximum_128_at_b16():
    case = su.case(128, B=16, n_steps=2, act_batch=17)
    eng = su.parity_check(case, n_more=1)
    su.act_check(eng, case, (1, 17))
    eng.close()


def test_84_at_b64_the_fast_head_shape():
    """whole 16-row blocks: the fast form of the head launch, conv3_bwd with riders where the plan finds empty slots"""
    su.parity_check(su.case(84, B=64, n_steps=2), n_more=1).close()


def test_graph_replay_equals_eager_at_50(monkeypatch):
    case = su.case(50, n_steps=4)
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv("GRL_NO_GRAPH", flag)
        eng = pu.engine_setup(case)
        eng.train(4, case["idx"], case["eps"])
        eng.train(3)
        out.append(su.state_of(eng))
        eng.close()
    assert su.same_state(*out)


def test_scalar_gather_fallback_at_36(monkeypatch):
    monkeypatch.setenv("GRL_NO_V2", "1")
    su.parity_check(su.case(36, n_steps=2), n_more=1).close()


@pytest.mark.parametrize("act_mfma", ["1", "0"])
def test_act_on_both_head_kernels_at_84(monkeypatch, capfd, act_mfma):
    monkeypatch.setenv("GRL_TUNE", "act_mfma=" + act_mfma)
    case = su.case(84, n_steps=1, act_batch=17)
    eng = pu.engine_setup(case)
    su.act_check(eng, case, (1, 17))
    eps = np.random.default_rng(5).standard_normal((17, 5)).astype(np.float32)
    from oracle import sac as osac
    st = case["stats"]
    obs = osac.normalize_obs(case["tr"]["obs"][:17], st["mean"], st["var"]).astype(np.float32)
    pu.close(eng.act(obs, False, eps), osac.SacOracle(case["spec"], case["params"]).act(obs, False, eps), what="stochastic action")
    eng.close()


def test_byte_colour_ring_at_50():
    case = su.case(50, "augmented_rgbd_u8", 8, n_steps=2)
    su.parity_check(case, n_more=1).close()


def test_behaviour_cloning_moves_the_policy_only_at_50():
    import bc_util as bu
    case = su.case(50, n_steps=1)
    rng = np.random.default_rng(1000)
    o = rng.integers(0, 256, case["tr"]["obs"].shape).astype(np.float32)
    o[..., -1] = 0.0
    o[:, 0, 0, -1] = rng.integers(0, 256, len(o))
    case.update(bc_batch=8, lr=1e-4, adam_eps=1e-8, low=-np.ones(5, np.float32), high=np.ones(5, np.float32), bc_obs=o,
                bc_act=rng.uniform(-1, 1, (len(o), 5)).astype(np.float32))
    idx = np.stack([rng.permutation(len(o))[:8] for _ in range(2)]).astype(np.int32)
    eng = pu.engine_setup(case)
    before = bu.arenas(eng)
    table = bu.begin(eng, case)
    eng.bc_train(table, idx)
    losses = eng.bc_losses()
    eng.bc_end()
    assert losses.shape == (2,) and np.isfinite(losses).all() and (losses > 0).all()
    bu.assert_only_trained_range_moved(eng, before, bu.arenas(eng))
    eng.close()
