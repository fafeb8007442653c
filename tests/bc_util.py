"""Behaviour-cloning pretraining on the engine (csrc/plan_bc.inl, csrc/bc_kernels.h) against a float64 restatement.

stable-baselines 2.10.1 `BaseRLModel.pretrain` with `SAC._get_pretrain_placeholders` is restated here over the oracle's own
network functions -- `oracle.sac.extractor_fwd / mlp_fwd / dense`, unchanged, fed float64 tensors -- with torch autograd:
    det = tanh(mu(obs));  a_env = low + 0.5 (det + 1)(high - low);  loss = mean over the n * A elements of (a_exp - a_env)^2
and `oracle.sac.adam_apply` (TF-1 Adam, float32) with `eps = adam_epsilon` as the optimiser.  The same helpers drive a handle of
the emulation build (tests/test_hostemu_bc.py) and of the device (tests/test_gpu_bc.py).

Tolerances are the project's (tests/parity_util.py): det and losses `close` (1e-5 + 1e-4 |ref|), every gradient tensor
`close_rel_max` (1e-3 max|g|); the optimiser is held to the engine's OWN fetched gradients through the restated Adam, every
trained parameter within 1e-6 absolute.  A ReLU unit whose float64 pre-activation lies within MARGIN of zero could take the other
side in float32: `assert_no_sign_ambiguity` looks at every unit of every row of the compared minibatch, on the restatement
alone and before anything is compared; the seeds of CASES were searched for (`find_seed`) so that none is that close."""
from collections import OrderedDict

import numpy as np
import torch

import parity_util as pu
from grasp_rl import synthetic
from oracle import sac as osac

MARGIN = 1e-5
N_ROWS = 40          # rows of every case's table

# name -> extractor / sizes / bc_batch / absent rows at the end of the compared update's index row / action bounds;
# data_seed: the first seed of the table at which the compared minibatch passes assert_no_sign_ambiguity (find_seed)
CASES = {
    "mlp_b8": dict(extractor="mlp", obs_dim=11, layers=(64, 64), A=5, B=32, bc_batch=8, seed=0),            # less than one 16-row block
    "mlp_b17_tail3": dict(extractor="mlp", obs_dim=11, layers=(64, 64), A=5, B=32, bc_batch=17, absent=3, seed=0),   # a block plus one row, three -1
    "mlp_b32": dict(extractor="mlp", obs_dim=11, layers=(64, 64), A=5, B=32, bc_batch=32, seed=0),
    "narrow_24_40": dict(extractor="mlp", obs_dim=11, layers=(24, 40), A=3, B=16, bc_batch=5, seed=0),      # widths that are no multiple of 16
    "wide_128_128": dict(extractor="mlp", obs_dim=11, layers=(128, 128), A=5, B=16, bc_batch=6, seed=0),
    "single_300": dict(extractor="mlp", obs_dim=11, layers=(300,), A=5, B=16, bc_batch=5, seed=0),
    "depth_augmented": dict(extractor="augmented", kind="depth", layers=(64, 64), A=5, B=8, bc_batch=8, seed=0, data_seed=1),
    "rgbd_augmented": dict(extractor="augmented", kind="rgbd", layers=(64, 64), A=5, B=8, bc_batch=4, seed=0),
    "depth_nature": dict(extractor="nature", kind="depth", layers=(64, 64), A=5, B=8, bc_batch=4, seed=0, data_seed=1),
    "asymmetric": dict(extractor="mlp", obs_dim=11, layers=(64, 64), A=5, B=16, bc_batch=7, seed=0,
                       low=(-1, -2, 0, -1, -0.5), high=(1, 2, 4, 1, 0.5)),
}
IMAGE_CASES = ("depth_augmented", "rgbd_augmented", "depth_nature")


def make_case(name, **over):
    a = dict(CASES[name], **over)
    kw = dict(extractor=a["extractor"], B=a["B"], n_replay=N_ROWS, act_dim=a["A"], layers=a["layers"], seed=a["seed"], n_steps=4)
    if a["extractor"] == "mlp":
        kw["obs_dim"] = a["obs_dim"]
    else:
        kw["kind"] = a["kind"]
    c = pu.make_case(**kw)               # a SAC case: configuration, parameters, a filled replay, statistics (never applied here)
    rng = np.random.default_rng(1000 + a.get("data_seed", 0))
    A, bb = a["A"], a["bc_batch"]
    low = np.asarray(a.get("low", (-1,) * A), np.float32)
    high = np.asarray(a.get("high", (1,) * A), np.float32)
    c.update(name=name, bc_batch=bb, low=low, high=high, lr=a.get("lr", 1e-4), adam_eps=a.get("adam_eps", 1e-8),
             bc_act=rng.uniform(low, high, (N_ROWS, A)).astype(np.float32))
    if a["extractor"] == "mlp":
        c["bc_obs"] = c["tr"]["obs"]
    else:
        # camera bytes in every image channel: pre-activations of order one (recorded depth / 255 is of order 1e-3, and
        # with it thousands of the 60 000 ReLU units of a row lie within MARGIN of zero)
        o = rng.integers(0, 256, c["tr"]["obs"].shape).astype(np.float32)
        if a["extractor"] == "augmented":
            o[..., -1] = 0.0
            o[:, 0, 0, -1] = rng.integers(0, 256, N_ROWS)
        c["bc_obs"] = o
    idx = np.stack([rng.permutation(N_ROWS)[:bb] for _ in range(3)]).astype(np.int32)
    if a.get("absent"):
        idx[0, bb - a["absent"]:] = -1
    c["bc_idx"] = idx                    # three updates; the first is the one held to the restatement
    return c


# --------------------------------------------------------------------------------------------------- the restatement
def _t64(P):
    return OrderedDict((k, torch.from_numpy(np.asarray(v, np.float64).copy())) for k, v in P.items())


def trained_names(spec):
    """model/pi without its log-std head: what the BC loss depends on."""
    return [n for n in osac.param_shapes(spec) if n.startswith("model/pi/") and "/dense_1/" not in n]


def prepare_obs(spec, obs):
    """The table's observations as the network sees them: used as held, images divided by 255 (float32, as the engine's
    input is), never normalised."""
    x = torch.from_numpy(np.asarray(obs, np.float32))
    if spec.extractor != "mlp":
        x = x / 255.0
    return x


def rows_of(idx_row):
    """table rows of one index row: an absent (-1) entry stands for row 0, which the loss masks"""
    return np.where(idx_row >= 0, idx_row, 0)


def forward64(spec, T, x, act, low, high, present):
    """det [n, A] and the loss over the `present` rows (float64 tensors)."""
    h = osac.extractor_fwd(spec, T, "model/pi", x.double())
    z = osac.mlp_fwd(spec, T, "model/pi", h)
    det = torch.tanh(osac.dense(T, "model/pi", "dense", z))
    lo, hi = torch.from_numpy(low.astype(np.float64)), torch.from_numpy(high.astype(np.float64))
    a_env = lo + 0.5 * (det + 1.0) * (hi - lo)
    sq = (torch.from_numpy(act.astype(np.float64)) - a_env) ** 2
    m = torch.from_numpy(np.asarray(present, np.float64))[:, None]
    return det, (sq * m).sum() / (m.sum() * sq.shape[1])


def preactivations64(spec, T, x):
    """Every ReLU pre-activation of pi's pass, float64, layer by layer (own arithmetic: the oracle's functions hand out
    activations only); checked against the oracle's activations where those are visible."""
    out = []
    x = x.double()
    if spec.extractor != "mlp":
        n1, n2, n3, nf = osac.cnn_names(spec)
        g = lambda n, s: T["model/pi/%s/%s:0" % (n, s)]
        img = x[..., :-1] if spec.extractor == "augmented" else x
        keep = {}
        h_ref = osac.extractor_fwd(spec, T, "model/pi", x, keep)
        cur = img
        for n, stride, k in ((n1, 4, "l1"), (n2, 2, "l2"), (n3, 1, "l3")):
            z = osac._conv_nhwc(cur, g(n, "w"), g(n, "b"), stride)
            out.append(z)
            cur = torch.relu(z)
            assert torch.equal(cur, keep[k])
        z = cur.reshape(cur.shape[0], -1) @ g(nf, "w") + g(nf, "b")
        out.append(z)
        h = h_ref
    else:
        h = x
    for i in range(len(spec.layers)):
        z = h @ T["model/pi/fc%d/kernel:0" % i] + T["model/pi/fc%d/bias:0" % i]
        out.append(z)
        h = torch.relu(z)
    assert torch.equal(h, osac.mlp_fwd(spec, T, "model/pi", osac.extractor_fwd(spec, T, "model/pi", x)))
    return out


def smallest_preactivation(case, P=None, idx_row=None):
    spec = case["spec"]
    rows = rows_of(case["bc_idx"][0] if idx_row is None else idx_row)
    T = _t64(case["params"] if P is None else P)
    with torch.no_grad():
        return min(float(z.abs().min()) for z in preactivations64(spec, T, prepare_obs(spec, case["bc_obs"][rows])))


def assert_no_sign_ambiguity(case, P=None, idx_row=None):
    m = smallest_preactivation(case, P, idx_row)
    assert m > MARGIN, "%s: a ReLU pre-activation of the float64 run lies %.2e from zero" % (case["name"], m)


def find_seed(name, tries=4000):
    """the first data seed at which the compared minibatch of `name` passes assert_no_sign_ambiguity"""
    for seed in range(tries):
        if smallest_preactivation(make_case(name, data_seed=seed)) > MARGIN:
            return seed
    raise AssertionError("no seed")


def reference_update(case, P, idx_row):
    """det, loss and the gradients of the trained variables at parameters P on one index row (float64)."""
    spec = case["spec"]
    rows, present = rows_of(idx_row), idx_row >= 0
    T = _t64(P)
    names = trained_names(spec)
    for n in names:
        T[n].requires_grad_(True)
    det, loss = forward64(spec, T, prepare_obs(spec, case["bc_obs"][rows]), case["bc_act"][rows], case["low"], case["high"], present)
    gs = torch.autograd.grad(loss, [T[n] for n in names])
    return det.detach().numpy(), float(loss.detach()), OrderedDict((n, g.numpy()) for n, g in zip(names, gs))


def reference_loss(case, P, idx_row):
    spec = case["spec"]
    rows = rows_of(idx_row)
    with torch.no_grad():
        return float(forward64(spec, _t64(P), prepare_obs(spec, case["bc_obs"][rows]), case["bc_act"][rows], case["low"], case["high"],
                               idx_row >= 0)[1])


def adam_state0(P, names):
    return osac.adam_init(P, names)


# --------------------------------------------------------------------------------------------------- the engine
def begin(eng, case, **over):
    eng.bc_begin(over.get("bc_batch", case["bc_batch"]), over.get("lr", case["lr"]), over.get("adam_eps", case["adam_eps"]),
                 case["low"], case["high"])
    return eng.bc_upload(case["bc_obs"], case["bc_act"])


def arenas(eng):
    """raw words of the state, replay and work arenas (parameters, SAC moments, DevScalars, statistics; the ring; the SAC
    update's workspace)"""
    return [np.array(eng.be.to_host(t), copy=True).view(np.uint32) for t in (eng.state, eng.replay, eng.work)]


def n_trained(eng):
    """the trained range is [0, offset of model/pi/dense_1/kernel:0) of the parameter block"""
    return [off for name, off, *_ in eng.table if name == "model/pi/dense_1/kernel:0"][0]


def assert_only_trained_range_moved(eng, before, after, moved=True):
    n = n_trained(eng)
    assert np.array_equal(before[0][n:], after[0][n:]), "state arena beyond the trained range changed"
    assert np.array_equal(before[1], after[1]), "replay arena changed"
    assert np.array_equal(before[2], after[2]), "work arena of the SAC plan changed"
    assert np.array_equal(before[0][:n], after[0][:n]) != moved


def route_from_dump(text):
    lines = sorted(set(l for l in text.splitlines() if l.startswith("grl plan: bc ")))
    assert len(lines) == 1, text
    return lines[0]


def check_update(eng, case):
    """One update of the case's first index row against the restatement; the optimiser against its own gradients; what must
    not move.  Returns the engine's parameters after the update."""
    spec, bb, A = case["spec"], case["bc_batch"], case["spec"].act_dim
    row = case["bc_idx"][0]
    assert_no_sign_ambiguity(case)
    det64, loss64, g64 = reference_update(case, case["params"], row)
    P0 = eng.get_parameters()
    before = arenas(eng)
    table = begin(eng, case)
    eng.bc_train(table, row[None])
    loss = eng.bc_losses()
    rows = rows_of(row)
    if spec.extractor != "mlp":
        Ci = spec.img_channels if spec.extractor == "augmented" else spec.obs_channels
        x = eng.fetch("bc_obs", (bb, 64, 64, Ci))
        assert np.array_equal(x, prepare_obs(spec, case["bc_obs"][rows]).numpy()[..., :Ci]), "the update's input is not bit-exact"
    else:
        ld = (spec.obs_dim + 3) // 4 * 4
        assert np.array_equal(eng.fetch("bc_obs", (bb, ld))[:, :spec.obs_dim], case["bc_obs"][rows])
    assert np.array_equal(eng.fetch("bc_act", (bb, A)), case["bc_act"][rows])
    pu.close(eng.fetch("bc_det", (bb, A)), det64, what="det")
    assert loss.shape == (1,)
    pu.close(loss, [loss64], what="loss")
    assert not eng.fetch("bc_dmu", (bb, (A + 3) // 4 * 4))[row < 0].any(), "an absent row has an output gradient"
    G = eng.get_gradients()
    for n, g in g64.items():
        pu.close_rel_max(G[n], g, what="grad " + n)
    # the optimiser on the engine's own gradients: fresh moments and beta powers, eps = adam_epsilon
    names = list(g64)
    Pref = OrderedDict((n, P0[n].copy()) for n in names)
    osac.adam_apply(Pref, OrderedDict((n, G[n]) for n in names), adam_state0(P0, names), case["lr"], eps=case["adam_eps"])
    P1 = eng.get_parameters()
    for n in P1:
        if n in Pref:
            d = np.abs(P1[n].astype(np.float64) - Pref[n].astype(np.float64)).max()
            assert d <= 1e-6, "Adam %s: max |d| %.3e" % (n, d)
            assert not np.array_equal(P1[n], P0[n]), n + " did not move"
        else:
            assert np.array_equal(P1[n], P0[n]), n + " is outside the trained set and changed"
    assert_only_trained_range_moved(eng, before, arenas(eng))
    # forward only: the loss at the new parameters, nothing moves
    mid = arenas(eng)
    eng.bc_eval(table, case["bc_idx"][1:3])
    ev = eng.bc_losses()
    pu.close(ev, [reference_loss(case, P1, r) for r in case["bc_idx"][1:3]], what="validation loss")
    assert all(np.array_equal(a, b) for a, b in zip(mid, arenas(eng))), "an evaluation moved something"
    eng.bc_end()
    return P1


def bc_snapshot(eng):
    return arenas(eng)[0]


def check_one_call_equals_single_calls(make_engine, case):
    snaps = []
    for split in (False, True):
        eng = make_engine()
        table = begin(eng, case)
        if split:
            for r in case["bc_idx"]:
                eng.bc_train(table, r[None])
        else:
            eng.bc_train(table, case["bc_idx"])
        losses = eng.bc_losses()
        m = eng.fetch("bc_adam_m")
        eng.bc_end()
        snaps.append((bc_snapshot(eng), m.view(np.uint32), losses.view(np.uint32)[-1:]))
        eng.close()
    for a, b in zip(*snaps):
        assert np.array_equal(a, b)


def check_second_session_starts_fresh(make_engine, case):
    """two identical sessions from identical parameters, on ONE handle, leave identical parameters"""
    eng = make_engine()
    out = []
    for _ in range(2):
        eng.set_parameters(case["params"])
        table = begin(eng, case)
        eng.bc_train(table, case["bc_idx"])
        eng.bc_end()
        out.append(bc_snapshot(eng))
    eng.close()
    assert np.array_equal(out[0], out[1])


def check_pretrain_then_train_equals_set_parameters_then_train(make_engine, case):
    """engine A: BC, then four SAC updates on given indices / noise; engine B: A's post-BC parameters, the same updates"""
    a = make_engine()
    table = begin(a, case)
    a.bc_train(table, case["bc_idx"])
    a.bc_end()
    P = a.get_parameters()
    a.train(4, case["idx"], case["eps"])
    b = make_engine()
    b.set_parameters(P)
    b.train(4, case["idx"], case["eps"])
    sa, sb = arenas(a), arenas(b)
    a.close()
    b.close()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])


def check_refusals_move_nothing(eng, case, other_handles=()):
    from grasp_rl._capi import GrlError
    import pytest
    before = arenas(eng)
    with pytest.raises(GrlError, match=r"batch %d exceeds the handle's batch_size %d" % (case["B"] + 1, case["B"])):
        begin(eng, case, bc_batch=case["B"] + 1)
    obs, act, n = eng.bc_upload(case["bc_obs"], case["bc_act"])
    with pytest.raises(GrlError, match="needs an open session"):
        eng._session = {"batch": case["bc_batch"], "keep": None}
        eng.bc_train((obs, act, n), case["bc_idx"])
    table = begin(eng, case)
    bad = case["bc_idx"].copy()
    bad[1, 2] = N_ROWS
    with pytest.raises(GrlError, match="index row 1, entry 2 is outside the table"):
        eng.bc_train(table, bad)
    bad = case["bc_idx"].copy()
    bad[2, 1] = -1
    with pytest.raises(GrlError, match="index row 2, entry 2 follows a -1"):
        eng.bc_train(table, bad)
    with pytest.raises(GrlError, match="a behaviour-cloning session is open"):
        begin(eng, case)
    eng.bc_end()
    assert all(np.array_equal(x, y) for x, y in zip(before, arenas(eng))), "a refused call moved something"


# --------------------------------------------------------------------------------------------------- learning (tests/test_gpu_bc_learn.py)
LEARN = dict(episodes=200, n_epochs=20, learning_rate=1e-4, adam_epsilon=1e-8, batch_size=64, layers=[64, 64], seed=0)


def record_reach_expert(episodes=LEARN["episodes"], seed=0):
    """ReachGraspEnv(kind="vector") driven by the expert that commands the object's position; the recorded arrays."""
    from grasp_rl.sb.expert import generate_expert_traj
    env = synthetic.ReachGraspEnv(kind="vector", seed=seed)
    expert = lambda obs: np.array([env._p[0], env._p[1], 0.0, 0.0, 0.0], np.float32)
    return env, generate_expert_traj(expert, None, env, n_episodes=episodes)


def reach_dataset(data):
    from grasp_rl.sb.expert import ExpertDataset
    np.random.seed(LEARN["seed"])        # the split and every epoch's shuffle
    return ExpertDataset(traj_data=data, batch_size=LEARN["batch_size"], verbose=0)


class RestatedPolicy:
    """The float64 restatement as a model evaluate_success can drive: pretrain over the loader's own minibatches, predict."""

    def __init__(self, spec, P, action_space):
        self.spec, self.P, self.action_space = spec, OrderedDict((n, np.array(v, np.float32)) for n, v in P.items()), action_space

    def pretrain(self, dataset, n_epochs, learning_rate, adam_epsilon, val_interval=None):
        names = trained_names(self.spec)
        st = adam_state0(self.P, names)
        case = {"spec": self.spec, "bc_obs": dataset.observations, "bc_act": dataset.actions, "low": self.action_space.low,
                "high": self.action_space.high}
        val_interval = val_interval or (1 if n_epochs < 10 else n_epochs // 10)
        for epoch in range(n_epochs):
            for row in dataset.train_loader.index_rows():
                _, _, G = reference_update(case, self.P, row)
                osac.adam_apply(self.P, {n: G[n].astype(np.float32) for n in names}, st, learning_rate, eps=adam_epsilon)
            if (epoch + 1) % val_interval == 0:
                dataset.val_loader.index_rows()      # (the engine's run draws this shuffle too)
        return self

    def predict(self, observation, state=None, mask=None, deterministic=True):
        x = torch.from_numpy(np.asarray(observation, np.float64).reshape(1, -1))
        T = _t64(self.P)
        with torch.no_grad():
            det = torch.tanh(osac.dense(T, "model/pi", "dense", osac.mlp_fwd(self.spec, T, "model/pi", x))).numpy()[0]
        low, high = self.action_space.low, self.action_space.high
        return np.clip(low + 0.5 * (det + 1.0) * (high - low), low, high).astype(np.float32), None
