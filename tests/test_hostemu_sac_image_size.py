"""SAC CnnPolicy on square images other than 64x64 (grl_config.img_hw 36 .. 128) through the C ABI on the g++ emulation build:
the launch plan with the geometry of the handle's image size -- buffer sizes, addressing tables, dense shapes, the parameter
table -- against the oracle's own arithmetic (tests/sac_image_size_util.py).

hw   o1 / o2 / o3   what it can break
36    8 /  3 /  1   the minimum: dense K = 64, one output pixel
50   11 /  4 /  2   borders that no window of conv1 / conv2 covers; row counts that are no multiple of 16
84   20 /  9 /  7   the customary Nature-CNN size, K = 3136
(128 runs on the device only: tests/test_gpu_sac_image_size.py)
"""
import numpy as np
import pytest

import bc_util as bu
import checkpoint_util as cu
import parity_util as pu
import sac_image_size_util as su
from grasp_rl import _capi
from grasp_rl.engine import SacEngine
from grasp_rl.init import init_parameters
from hostemu_backend import NumpyHostBackend
from oracle import sac as osac

NOTE = "grl plan: sac image %dx%d per-layer convolutions (conv_stack is 64x64 only)"


@pytest.fixture(scope="module")
def emu(hostemu_lib, request):
    import os
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _kw(lib):
    return dict(backend=NumpyHostBackend(), lib_path=lib)


def test_the_helper_table_is_the_oracles_at_64():
    """Before anything relies on the helper: at 64x64 its shape table and its seeded parameters are the oracle's, entry for entry."""
    for kw in su.PARITY.values():
        C = 2 if kw["kind"] == "depth" else 5
        aug = kw["extractor"] == "augmented"
        spec = osac.SacSpec(extractor=kw["extractor"], img_hw=64, img_channels=C - 1 if aug else C, n_direct=1 if aug else 0)
        mine, ref = su.param_shapes(spec), osac.param_shapes(spec)
        assert list(mine.items()) == list(ref.items())
        Pm, Pr = su.init_params(spec, 3), osac.init_params(spec, 3)
        assert list(Pm) == list(Pr) and all(Pm[n].dtype == Pr[n].dtype and np.array_equal(Pm[n], Pr[n]) for n in Pr)
        assert osac.param_shapes(spec) == ref           # (the oracle's own function is back in place)
    assert [su.geometry(hw) for hw in (36, 50, 64, 84, 128)] == [(8, 3, 1), (11, 4, 2), (15, 6, 4), (20, 9, 7), (31, 14, 12)]
    assert su.dense_k(64) == 1024 and su.dense_k(84) == 3136 and su.dense_k(128) == 9216 and su.dense_k(36) == 64
    assert su.geometry(35)[2] < 1


@pytest.mark.parametrize("key", sorted(su.DATA_SEED), ids=lambda k: "%d-%s-b%d" % k)
def test_the_seed_of_every_case_keeps_relu_units_off_zero(key):
    """On the oracle alone, before anything is compared: no ReLU unit of the compared minibatch lies within the frozen
    ambiguity tolerance of zero, so no comparison of these files needs (or has) a second look with the engine's signs."""
    su.assert_no_sign_ambiguity(su.case(*key, n_steps=2))


@pytest.mark.parametrize("name", list(su.PARITY))
@pytest.mark.parametrize("hw", [36, 50, 84])
def test_update_and_act_match_the_oracle(emu, monkeypatch, capfd, hw, name):
    case = su.case(hw, name, 8, n_steps=4, act_batch=17)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    eng = su.parity_check(case, n_more=3, **_kw(emu))          # first step against the oracle, then three updates
    dump = capfd.readouterr().err
    monkeypatch.delenv("GRL_PLAN_DUMP")
    assert NOTE % (hw, hw) in dump, dump
    assert "conv_stack_fwd" not in dump and "conv_stack_bwd" not in dump
    for tag in ("conv1_fwd", "conv2_fwd", "conv3_fwd", "conv3_bwd", "conv2_bwd", "wgrad_conv"):
        assert tag in dump, tag
    k = su.dense_k(hw)
    assert [tuple(t[3]) for t in eng.table if t[0].endswith(("cnn_fc1/w:0", "/fc1/w:0"))] == [(k, 512)] * 3
    su.act_check(eng, case, (1, 17))
    eng.close()


@pytest.mark.parametrize("name", list(su.PARITY))
@pytest.mark.parametrize("hw", [36, 50, 84])
def test_a_call_of_three_updates_equals_three_calls(emu, hw, name):
    case = su.case(hw, name, 8, n_steps=1)
    out = []
    for split in ([3], [1, 1, 1]):
        eng = pu.engine_setup(case, **_kw(emu))
        for n in split:
            eng.train(n)
        out.append(su.state_of(eng) + [eng.fetch("idx_raw").copy()])
        assert eng.metrics() == eng.metrics()
        eng.close()
    assert su.same_state(*out)


@pytest.mark.parametrize("name", list(su.PARITY))
@pytest.mark.parametrize("hw", [36, 50, 84])
def test_optimiser_step_on_identical_inputs(emu, hw, name):
    pu.check_optimiser_steps(su.case(hw, name, 8, n_steps=2), n=2, **_kw(emu))


def test_byte_colour_ring_at_50(emu):
    case = su.case(50, "augmented_rgbd_u8", 8, n_steps=2)
    su.parity_check(case, n_more=1, **_kw(emu)).close()


def test_observe_once_with_device_statistics_at_50(emu):
    """normalize = 1 and grl_observe on 50x50x2 observations: acting on the observed copy, the ring rows it writes and the
    running statistics are bit-identical to the separate uploads (grl_norm_update, grl_act, grl_replay_add)."""
    n, shape = 5, (50, 50, 2)
    cfg = lambda: _capi.make_config("augmented", obs_channels=2, n_direct=1, act_dim=5, layers=(64, 64), batch_size=4,
                                    replay_capacity=12, normalize=True, act_batch=n, img_hw=50)
    a, b = SacEngine(cfg(), **_kw(emu)), SacEngine(cfg(), **_kw(emu))
    assert int(a.cfg.normalize) == 1
    p = init_parameters(a.table, seed=2)
    a.set_parameters(p); b.set_parameters(p)
    rng = np.random.default_rng(11)

    def draw(k):
        x = rng.uniform(0.0, 1.0, (k,) + shape).astype(np.float32)
        x[..., -1] = 0.0
        x[:, 0, 0, -1] = rng.uniform(0, 1, k)
        return x
    obs = draw(n)
    a.norm_update(obs)
    b.observe(obs, update_stats=True)
    for step in range(4):
        eps = rng.standard_normal((n, 5)).astype(np.float32)
        det = step % 2 == 0
        act_a = a.act(obs, deterministic=det, eps=None if det else eps, raw=True)
        act_b = b.act(n, deterministic=det, eps=None if det else eps, raw=True, observed=True)
        assert np.array_equal(act_a, act_b), step
        new, rew = draw(n), rng.normal(size=n).astype(np.float32)
        done = (rng.uniform(size=n) < 0.4).astype(np.float32)
        rows = [i for i in range(n) if done[i] > 0]
        term = draw(len(rows)) if rows else None
        store = new.copy()
        for j, i in enumerate(rows):
            store[i] = term[j]
        a.norm_update(new)
        a.replay_add(obs, act_a, rew, store, done)
        b.observe(new, update_stats=True)
        b.replay_add_observed(act_b, rew, done, rows, term)
        obs = new
    for name in ("rp_obs", "rp_next", "rp_dobs", "rp_dnext", "rp_act", "rp_rew", "rp_done"):     # (12 slots, 20 transitions: wrapped)
        ra, rb = a.fetch(name), b.fetch(name)
        assert ra.shape == rb.shape and np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), name
    ma, mb = a.get_obs_stats(shape), b.get_obs_stats(shape)
    assert ma[2] == mb[2] and abs(ma[2] - 5 * n) < 1e-3 and np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    a.train(2); b.train(2)                                       # and the updates that read those rows and statistics
    assert su.same_state(su.state_of(a), su.state_of(b))
    a.close(); b.close()


def test_behaviour_cloning_moves_the_policy_only_at_50(emu):
    case = su.case(50, n_steps=1)
    rng = np.random.default_rng(1000)
    o = rng.integers(0, 256, case["tr"]["obs"].shape).astype(np.float32)
    o[..., -1] = 0.0
    o[:, 0, 0, -1] = rng.integers(0, 256, len(o))
    case.update(bc_batch=8, lr=1e-4, adam_eps=1e-8, low=-np.ones(5, np.float32), high=np.ones(5, np.float32), bc_obs=o,
                bc_act=rng.uniform(-1, 1, (len(o), 5)).astype(np.float32))
    idx = np.stack([rng.permutation(len(o))[:8] for _ in range(2)]).astype(np.int32)
    eng = pu.engine_setup(case, **_kw(emu))
    P0, before = eng.get_parameters(), bu.arenas(eng)
    table = bu.begin(eng, case)
    eng.bc_train(table, idx)
    losses = eng.bc_losses()
    assert np.array_equal(eng.fetch("bc_obs", (8, 50, 50, 1)), (o[idx[1]] / np.float32(255.0))[..., :1])
    eng.bc_end()
    assert losses.shape == (2,) and np.isfinite(losses).all() and (losses > 0).all()
    bu.assert_only_trained_range_moved(eng, before, bu.arenas(eng))
    P1 = eng.get_parameters()
    trained = set(bu.trained_names(case["spec"]))
    for n in P1:
        assert np.array_equal(P1[n], P0[n]) == (n not in trained), n
    eng.close()


class _Run(cu.SacRun):
    def __init__(self, backend_factory, lib_path, case):
        self.case, self.backend_factory, self.lib_path = case, backend_factory, lib_path


def test_checkpoint_destroy_restore_continue_at_50(emu, tmp_path):
    run = _Run(NumpyHostBackend, emu, su.case(50, n_steps=1))
    a, b, _ = cu.continuation(run, str(tmp_path / "ck"), 3, poison=True)
    cu.assert_same_training_state(a, b, "50x50")
    a.close(); b.close()


@pytest.mark.parametrize("hw", [35, 129, 0])
def test_sizes_outside_36_to_128_are_refused_by_name(emu, hw):
    cfg = _capi.make_config("augmented", obs_channels=2, n_direct=1, batch_size=4, replay_capacity=8, img_hw=hw)
    with pytest.raises(_capi.GrlError, match=r"img_hw %d: square images of 36x36 to 128x128" % hw):
        SacEngine(cfg, **_kw(emu))


def test_a_buffer_past_the_32_bit_tables_is_refused(emu):
    """128x128x5 at batch 65536 would need 5.4e9 elements in an image buffer: refused at grl_query_sizes, nothing overflows."""
    cfg = _capi.make_config("augmented", obs_channels=5, n_direct=1, batch_size=65536, replay_capacity=8, img_hw=128)
    with pytest.raises(_capi.GrlError, match="32-bit offsets"):
        SacEngine(cfg, **_kw(emu))
