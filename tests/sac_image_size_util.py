"""Shared pieces of the SAC image-size tests (square camera images of 36x36 .. 128x128 through CnnPolicy).

The reference arithmetic is the oracle's own (oracle/sac.py): `extractor_fwd` reshapes whatever conv3 yields, only the shape
table `param_shapes` fixes the extractor's dense kernel at (1024, 512).  `param_shapes` / `init_params` here wrap the oracle's
with that one entry taken from the image size; tests/test_hostemu_sac_image_size.py first shows that at 64x64 they return what
the oracle returns, entry for entry, before anything else relies on them.

Tolerances are those of tests/parity_util.py (minibatch tensors bit-exact, forward 1e-5 + 1e-4 relative, gradients 1e-3 of the
per-tensor max, the optimiser through `check_apply_step`).  `compare_first_step` is parity_util's with the image geometry of the
case -- and WITHOUT its second look at sign-ambiguous ReLU units: the seeds of these cases are chosen so that none occurs.
"""
from collections import OrderedDict

import numpy as np

import parity_util as pu
from fake_env import FakeGraspEnv
from grasp_rl import _capi, synthetic
from grasp_rl.sb.spaces import Box
from oracle import sac as osac


def geometry(hw):
    """(o1, o2, o3): output sides of the three VALID convolutions (8x8 / 4, 4x4 / 2, 3x3 / 1) over a hw x hw image."""
    o1 = (hw - 8) // 4 + 1
    o2 = (o1 - 4) // 2 + 1
    return o1, o2, o2 - 2


def dense_k(hw):
    return 64 * geometry(hw)[2] ** 2


_ORACLE_PARAM_SHAPES = osac.param_shapes


def param_shapes(spec):
    """oracle.sac.param_shapes with the extractor's dense kernel sized by spec.img_hw."""
    out = _ORACLE_PARAM_SHAPES(spec)
    names = osac.cnn_names(spec)
    if names:
        for name in out:
            if name.endswith("/%s/w:0" % names[3]):
                out[name] = (dense_k(spec.img_hw), 512)
    return out


def init_params(spec, seed=0):
    """oracle.sac.init_params drawing over the table above (the oracle's own code, reading this module's table)."""
    saved = osac.param_shapes
    osac.param_shapes = param_shapes
    try:
        return osac.init_params(spec, seed)
    finally:
        osac.param_shapes = saved


def obs_stats(kind, hw):
    """The shipped 64x64 per-pixel statistics resampled (nearest pixel) to hw x hw; pixel [0, 0] -- which carries the direct
    feature in the pad channel -- maps to itself."""
    st = synthetic.load_obs_stats(kind)
    ii = (np.arange(hw) * 64) // hw
    pick = lambda a: np.ascontiguousarray(a[ii][:, ii])
    return {"mean": pick(st["mean"]), "var": pick(st["var"]), "ret_var": st["ret_var"], "count": st["count"]}


def make_case(hw, extractor="augmented", kind="depth", B=8, n_replay=24, act_dim=5, layers=(64, 64), seed=0, normalize=True,
              n_steps=2, rgb_u8=False, act_batch=4, data_seed=None):
    """data_seed: seed of the replay contents, minibatch indices and noise (default: `seed`, which also draws the parameters)"""
    stats = obs_stats(kind, hw)
    data_seed = seed if data_seed is None else data_seed
    tr = synthetic.make_transitions(n_replay, kind, act_dim, data_seed, stats)
    C = stats["mean"].shape[-1]
    if extractor == "augmented":
        spec = osac.SacSpec(extractor="augmented", img_hw=hw, img_channels=C - 1, n_direct=1, act_dim=act_dim, layers=list(layers))
    else:
        spec = osac.SacSpec(extractor="nature", img_hw=hw, img_channels=C, n_direct=0, act_dim=act_dim, layers=list(layers))
    cfg = _capi.make_config(extractor, obs_channels=C, n_direct=1 if extractor == "augmented" else 0, act_dim=act_dim,
                            layers=layers, batch_size=B, replay_capacity=n_replay, normalize=normalize, act_batch=act_batch,
                            replay_rgb_u8=rgb_u8, img_hw=hw)
    idx, eps = synthetic.make_noise(n_steps, B, act_dim, n_replay, data_seed + 1)
    return {"B": B, "n_steps": n_steps, "extractor": extractor, "normalize": normalize, "hw": hw, "spec": spec, "cfg": cfg,
            "stats": stats, "tr": tr, "idx": idx, "eps": eps, "params": init_params(spec, seed)}


class SizedGraspEnv(FakeGraspEnv):
    """tests/fake_env.py's image environment with a hw x hw camera (the reference: config/camera_info.yaml height / width,
    sensor.py:36-41): Box(0, 255, (hw, hw, C)), observations drawn from the resampled statistics."""

    def __init__(self, hw, kind="depth", **kw):
        super().__init__(kind, **kw)
        self.stats = obs_stats(kind, hw)
        self.observation_space = Box(0, 255, shape=self.stats["mean"].shape, dtype=np.float32)


# the parity cases of both files: extractor `augmented` on depth (1 + 1 channels), `nature` on RGB-D
PARITY = {"augmented_depth": dict(extractor="augmented", kind="depth"), "nature_rgbd": dict(extractor="nature", kind="rgbd")}


def relu_margin(case):
    """Smallest |pre-activation| over every ReLU unit the compared update differentiates through -- conv1..3 and the dense layer
    of both trained extractors, the hidden layers of pi, vf, qf1 and qf2 -- on the oracle's own float32 arithmetic, for the
    FIRST minibatch of the case.  A unit within parity_util.AMBIG_TOL_FROZEN of zero has no defined side in float32."""
    import torch
    spec = case["spec"]
    P = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in case["params"].items()}
    ii = case["idx"][0]
    raw = {k: case["tr"][k][ii] for k in ("obs", "act", "rew", "next_obs", "done")}
    nm = case["normalize"]
    b = osac.prepare_batch(spec, raw, case["stats"] if nm else None)
    n1, n2, n3, nf = osac.cnn_names(spec)
    low = float("inf")

    def hidden(h, scope):
        m = float("inf")
        for i in range(len(spec.layers)):
            z = h @ P["%s/fc%d/kernel:0" % (scope, i)] + P["%s/fc%d/bias:0" % (scope, i)]
            m, h = min(m, float(z.abs().min())), torch.relu(z)
        return m
    for scope in ("model/pi", "model/values_fn"):
        x = b["obs"]
        cur = x[..., :-1] if spec.extractor == "augmented" else x
        for n, s in ((n1, 4), (n2, 2), (n3, 1)):
            z = osac._conv_nhwc(cur, P["%s/%s/w:0" % (scope, n)], P["%s/%s/b:0" % (scope, n)], s)
            low, cur = min(low, float(z.abs().min())), torch.relu(z)
        z = cur.reshape(cur.shape[0], -1) @ P["%s/%s/w:0" % (scope, nf)] + P["%s/%s/b:0" % (scope, nf)]
        low = min(low, float(z.abs().min()))
        feat = osac.extractor_fwd(spec, P, scope, x)
        if scope == "model/pi":
            low = min(low, hidden(feat, "model/pi"))
        else:
            low = min(low, hidden(feat, scope + "/vf"), hidden(torch.cat([feat, b["act"]], 1), scope + "/qf1"),
                      hidden(torch.cat([feat, b["act"]], 1), scope + "/qf2"))
    return low


def assert_no_sign_ambiguity(case):
    m = relu_margin(case)
    assert m > pu.AMBIG_TOL_FROZEN, "a ReLU pre-activation of the oracle's run lies %.2e from zero" % m


def find_data_seed(tries=5000, **kw):
    """the first data seed at which the case passes assert_no_sign_ambiguity (how the data_seed of the cases below was found)"""
    for s in range(tries):
        if relu_margin(make_case(data_seed=s, **kw)) > pu.AMBIG_TOL_FROZEN:
            return s
    raise AssertionError("no seed")


# (hw, parity case, B) -> the first data seed at which the compared minibatch has no ReLU unit within AMBIG_TOL_FROZEN of zero
# (find_data_seed; tests/test_hostemu_sac_image_size.py asserts it for every entry, on the oracle alone)
N_REPLAY = {8: 24, 16: 32, 64: 96}
DATA_SEED = {(36, "augmented_depth", 8): 0, (36, "nature_rgbd", 8): 1, (50, "augmented_depth", 8): 1, (50, "nature_rgbd", 8): 0,
             (84, "augmented_depth", 8): 2, (84, "nature_rgbd", 8): 1, (128, "augmented_depth", 16): 22,
             (84, "augmented_depth", 64): 310, (50, "augmented_rgbd_u8", 8): 0}


def case(hw, name="augmented_depth", B=8, **kw):
    """The parity case (hw, name, B) on its searched data seed."""
    base = dict(extractor="augmented", kind="rgbd", rgb_u8=True) if name == "augmented_rgbd_u8" else PARITY[name]
    return make_case(hw, B=B, n_replay=N_REPLAY[B], data_seed=DATA_SEED[(hw, name, B)], **base, **kw)


def compare_first_step(eng, case, d0):
    """parity_util.compare_first_step for the image size of the case; a gradient mismatch is a failure (no ReLU hints)."""
    spec, B, A, hw = case["spec"], case["B"], case["spec"].act_dim, case["hw"]
    batch = d0["batch"]
    ldf = (spec.feat_dim + 3) // 4 * 4
    Ci = spec.img_channels if spec.extractor == "augmented" else spec.obs_channels
    assert np.array_equal(eng.fetch("x_obs", (B, hw, hw, Ci)), batch["obs"].numpy()[..., :Ci]), "normalised obs minibatch is not bit-exact"
    assert np.array_equal(eng.fetch("x_next", (B, hw, hw, Ci)), batch["next_obs"].numpy()[..., :Ci]), "normalised next_obs minibatch is not bit-exact"
    assert np.array_equal(eng.fetch("rew", (B,)), batch["rew"].numpy()), "normalised reward not bit-exact"
    assert np.array_equal(eng.fetch("done", (B,)), batch["done"].numpy())
    assert np.array_equal(eng.fetch("act", (B, A)), batch["act"].numpy())
    F = spec.feat_dim
    for name, key in (("feat_pi", "h_pi"), ("feat_vf", "h_c"), ("feat_tgt", "h_tgt")):
        pu.close(eng.fetch(name, (B, ldf))[:, :F], d0[key], what=name)
    for name in ("mu", "pi"):
        pu.close(eng.fetch(name, (B, A)), d0[name], what=name)
    pu.close(np.clip(eng.fetch("log_std", (B, A)), osac.LOG_STD_MIN, osac.LOG_STD_MAX), d0["log_std"], what="log_std")
    for name in ("logp", "qf1", "qf2", "v", "v_tgt", "qf1_pi", "qf2_pi"):
        pu.close(eng.fetch(name, (B,)), d0[name], atol=2e-5, rtol=2e-4, what=name)
    m = eng.metrics()
    for k_e, k_o in (("policy_loss", "policy_loss"), ("qf1_loss", "qf1_loss"), ("qf2_loss", "qf2_loss"),
                     ("value_loss", "value_loss"), ("ent_coef_loss", "ent_loss"), ("ent_coef", "ent_coef")):
        ref = float(d0[k_o])
        assert abs(m[k_e] - ref) <= 1e-4 * abs(ref) + 1e-6, (k_e, m[k_e], ref)
    G = eng.get_gradients()
    assert set(G) == set(d0["grads"])
    for n, g in d0["grads"].items():
        pu.close_rel_max(G[n], g, what="grad " + n)


def parity_check(case, n_more=3, **engine_kw):
    """First update against the oracle (tensors, losses, gradients), n_more further updates against its parameters and
    moments; returns the engine for further checks (the caller closes it)."""
    n = 1 + n_more
    assert case["n_steps"] >= n
    ref, orc = pu.oracle_run(case)
    eng = pu.engine_setup(case, **engine_kw)
    eng.train(1, case["idx"][:1], case["eps"][:1])
    compare_first_step(eng, case, ref[0])
    if n_more:
        eng.train(n_more, case["idx"][1:n], case["eps"][1:n])
    pu.compare_params(eng, orc, case["spec"].lr, n)
    return eng


def act_check(eng, case, rows_list=(1, 17)):
    """Deterministic actions for the given row counts against the oracle (forward tolerance)."""
    orc = osac.SacOracle(case["spec"], eng.get_parameters())
    st = case["stats"]
    cap = case["cfg"].act_batch
    for rows in rows_list:
        raw = np.concatenate([case["tr"]["obs"]] * (rows // len(case["tr"]["obs"]) + 1))[:rows]
        obs = osac.normalize_obs(raw, st["mean"], st["var"]).astype(np.float32)
        got = np.concatenate([eng.act(obs[k:k + cap], True) for k in range(0, rows, cap)])
        pu.close(got, orc.act(obs, True), what="deterministic action, %d rows" % rows)


def state_of(eng):
    """Everything an update moves, for bit-for-bit comparisons."""
    P = eng.get_parameters()
    return [P[n] for n in P] + [eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy()]


def same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
