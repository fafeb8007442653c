"""DQN / BDQ engine-vs-oracle comparison shared by the CPU plan test and the GPU parity test."""
import numpy as np
import torch

import parity_util as pu
from grasp_rl import _capi
from grasp_rl.engine import QEngine
from oracle import dqn as od

CASES = {
    "dqn": dict(algo="dqn", obs_dim=20, D=1, bins=6, common=(), branch=(16, 16), value=(16, 16), B=8),
    "dqn_reference_shape": dict(algo="dqn", obs_dim=100, D=1, bins=12, common=(), branch=(64, 64), value=(64, 64), B=32),
    "bdq": dict(algo="bdq", obs_dim=20, D=3, bins=5, common=(16, 16), branch=(8,), value=(8,), B=8),
    "bdq_5_branches": dict(algo="bdq", obs_dim=24, D=5, bins=7, common=(32, 16), branch=(8,), value=(12,), B=9),
    "bdq_reference_shape": dict(algo="bdq", obs_dim=100, D=3, bins=33, common=(64, 64), branch=(32,), value=(32,), B=64),
    # BASELINE configs[2] exactly: gripper_grasp.yaml:104-118 (layers [[64,64],[32],[32]], num_actions_pad 33,
    # batch 64) on the 101-d auto-encoder observation (100 features + gripper width), 5 action dimensions
    "bdq_baseline_config3": dict(algo="bdq", obs_dim=101, D=5, bins=33, common=(64, 64), branch=(32,), value=(32,), B=64, lr=1e-4),
    # ... and as gripper_grasp.yaml:104-118 actually selects it: `prioritized_replay: False` (:106) -- uniform replay, every
    # importance weight 1
    "bdq_baseline_config3_uniform": dict(algo="bdq", obs_dim=101, D=5, bins=33, common=(64, 64), branch=(32,), value=(32,), B=64,
                                         lr=1e-4, uniform=True),
    # the alternative readings of the unavailable bdq_sb fork (oracle/dqn.py switches): TD loss summed over the
    # branches; no 1/(D+1) rescaling of the trunk gradient
    "bdq_loss_sum": dict(algo="bdq", obs_dim=20, D=3, bins=5, common=(16, 16), branch=(8,), value=(8,), B=8, loss_sum=True),
    "bdq_no_trunk_rescale": dict(algo="bdq", obs_dim=20, D=3, bins=5, common=(16, 16), branch=(8,), value=(8,), B=8,
                                 trunk_rescale=False),
}


# ---------------------------------------------------------------------------------------------------
# Shapes on BOTH sides of every decision csrc/plan_q.inl / csrc/q_act.h take by shape alone (tests/test_gpu_q_shapes.py on
# the MI355X, tests/test_hostemu_q_shapes.py on the emulation build).  `route` is the kernel set the case exists for, written
# down from the conditions in the sources (restated in planned_route below), never from what the engine prints:
#   chains   row-local chains (q_kernels.h / q_mfma.h) instead of one GEMM launch per layer
#   mfma     ... on the matrix-core stages (q_mfma.h); without it the VALU stages of q_kernels.h
#   l0       ... with layer 0 inside the chain (no q_l0 GEMM launch in front)
#   chained  loss + weight gradients inside the backward chains (q_chain.h)
#   apply    reduction + clip + Adam as one launch (q_apply_kernels.h)
#   q_pf     multi-update uniform calls with draw + gather on the apply launch
#   act      one-launch epsilon-greedy act (q_act.h); without it the launch list + q_select_kernel
_ALL = "chains mfma l0 chained apply q_pf act"
_S = dict(algo="bdq", obs_dim=30, common=(32,), branch=(16,), value=(16,), B=16)       # the small network the edge cases vary
SHAPE_CASES = {
    # width 128 == HT_MAXW exactly, trunk end 64 == HT_MAXA exactly: the widest network the VALU chains take
    "valu_w128": dict(algo="bdq", obs_dim=100, D=3, bins=33, common=(128, 64), branch=(96,), value=(72,), B=24,
                      route="chains apply q_pf"),
    # one unit past the matrix-core stages' 64 in ONE tower only (added: the 64 | 65 edge itself; valu_w128 is far from it)
    "valu_w65": dict(_S, D=3, bins=5, common=(64, 64), branch=(65,), value=(64,), route="chains apply q_pf"),
    "gemm_trunk_end_128": dict(algo="bdq", obs_dim=100, D=3, bins=33, common=(128, 128), branch=(32,), value=(32,), B=24,
                               route="apply"),       # 128 x 128: a variable of exactly GRL_QAPPLY_MAX floats on the GEMM path
    # trunk end 65 == HT_MAXA + 1 (added: the edge itself)
    "gemm_trunk_end_65": dict(_S, D=3, bins=5, common=(32, 65), route="apply"),
    "gemm_w130": dict(algo="bdq", obs_dim=40, D=2, bins=9, common=(130, 48), branch=(20,), value=(20,), B=17, route="apply"),
    # trained_models/BDQ_33pads_big: K = 512 GEMMs, a 131072-float variable through the three-launch apply
    "shipped_big": dict(algo="bdq", obs_dim=100, D=3, bins=33, common=(512, 256), branch=(128,), value=(128,), B=32, route=""),
    "obs128": dict(algo="bdq", obs_dim=128, D=3, bins=33, common=(64, 64), branch=(32,), value=(32,), B=32, route=_ALL),
    "obs129": dict(algo="bdq", obs_dim=129, D=3, bins=33, common=(64, 64), branch=(32,), value=(32,), B=32,
                   route="chains mfma apply q_pf"),
    "obs300": dict(algo="dqn", obs_dim=300, D=1, bins=12, common=(), branch=(64, 64), value=(64, 64), B=32, route="chains mfma"),
    "qapply_edge": dict(algo="dqn", obs_dim=100, D=1, bins=12, common=(), branch=(128, 128), value=(128, 128), B=32,
                        route="chains apply q_pf"),  # 128 x 128 == GRL_QAPPLY_MAX exactly
    # 129 x 128 = GRL_QAPPLY_MAX + 128 (added: the smallest step past the edge these widths allow; obs300 is 19200)
    "qapply_over": dict(algo="dqn", obs_dim=129, D=1, bins=12, common=(), branch=(128, 128), value=(128, 128), B=32,
                        route="chains"),
    "bins64_D4": dict(_S, D=4, bins=64, route=_ALL),                                         # D * bins == 256
    "bins64_D5": dict(_S, D=5, bins=64, route="chains mfma l0 apply q_pf act"),              # D * bins == 320
    "bins65": dict(_S, D=2, bins=65, route="apply"),
    "D7": dict(_S, D=7, bins=5, route=_ALL),                                                 # D + 1 == QM_MAXP
    "D8": dict(_S, D=8, bins=5, route="chains apply q_pf"),
    "depth_2_2_1": dict(_S, D=3, bins=5, common=(32, 24), branch=(16, 12), value=(20,), route=_ALL),     # Lb > Lv
    "depth_2_1_2": dict(_S, D=3, bins=5, common=(32, 24), branch=(16,), value=(20, 10), route=_ALL),     # Lb < Lv
    "depth_3_2": dict(_S, D=2, bins=5, common=(32, 24, 16), branch=(16, 8), value=(8,), route="apply"),  # depth sum 5
    "depth_3_1": dict(_S, D=2, bins=5, common=(32, 24, 16), branch=(16,), value=(8,), route=_ALL),       # depth sum 4
    "depth_0_4": dict(_S, algo="dqn", D=1, bins=5, common=(), branch=(16, 12, 10, 8), value=(16, 12, 10, 8), route=_ALL),
    # no trunk AND towers of unequal depth (added: q_act.h names this hand-over -- the value chain starts from the observation)
    "depth_0_3_1": dict(_S, algo="dqn", D=1, bins=5, common=(), branch=(16, 12, 10), value=(20,), route=_ALL),
    "odd_widths": dict(algo="bdq", obs_dim=7, D=3, bins=3, common=(17, 5), branch=(3,), value=(1,), B=5, route=_ALL),
    "B1": dict(CASES["bdq"], B=1, route=_ALL),
    "B_ref_ragged": dict(CASES["bdq_baseline_config3"], B=50, route=_ALL),                   # last row block: 2 of 16 rows
    "B1040": dict(CASES["bdq"], B=1040, n_replay=1100, route="chains mfma l0 chained apply act"),
}
del _S, _ALL


def case_args(name, **over):
    """make_q_case arguments of a case of either table."""
    a = dict(CASES[name] if name in CASES else SHAPE_CASES[name])
    a.pop("route", None)
    a.update(over)
    return a


def declared_route(name):
    return frozenset(SHAPE_CASES[name]["route"].split())


def trainable_sizes(a):
    """floats of every kernel matrix of the online network (the biases are smaller)"""
    out, k = [], a["obs_dim"]
    for w in a["common"]:
        out.append(k * w)
        k = w
    for hidden, n_out, copies in ((a["branch"], a["bins"], a["D"]), (a["value"], 1, 1)):
        kk = k
        for w in tuple(hidden) + (n_out,):
            out += [kk * w] * copies
            kk = w
    return out


def planned_route(a):
    """The routing conditions of csrc/plan_q.inl (fused_q, want_mfma, l0_chain, qapply_feasible, q_chain, q_pf) and
    csrc/q_act.h (qa_shape_ok) on an MI355X with no GRL_TUNE switch set, restated: HT_MAXW 128, HT_MAXA 64, QM_W 64,
    QM_MAXP 8, QC_XW 128, GRL_MAX_LAYERS 4, GRL_QAPPLY_MAX 16384."""
    widths = tuple(a["common"]) + tuple(a["branch"]) + tuple(a["value"])
    depth = len(a["common"]) + max(len(a["branch"]), len(a["value"]))
    D, bins, obs = a["D"], a["bins"], a["obs_dim"]
    r = set()
    chains = bins <= 64 and depth <= 4 and max(widths) <= 128 and (not a["common"] or a["common"][-1] <= 64)
    mfma = chains and max(widths) <= 64 and D + 1 <= 8
    apply_ = max(trainable_sizes(a)) <= 16384
    for flag, on in (("chains", chains), ("mfma", mfma), ("l0", mfma and obs <= 128),
                     ("chained", mfma and apply_ and D * bins <= 256 and obs <= 128), ("apply", apply_),
                     ("q_pf", chains and apply_ and a["B"] <= 1024),
                     ("act", obs <= 128 and D <= 7 and bins <= 64 and max(widths) <= 64 and depth <= 4)):
        if on:
            r.add(flag)
    return frozenset(r)


def route_from_dump(plan, matrix_cores=True):
    """The route a GRL_PLAN_DUMP=1 text reports.  matrix_cores=False: the emulation build, which always runs the VALU form of
    the forward chains (and so says nothing about `mfma` / `l0`)."""
    assert ("grl plan: q chains" in plan) != ("grl plan: q_fwd" in plan), plan          # chains XOR per-layer GEMM launches
    assert ("in one launch: yes" in plan) != ("in one launch: no" in plan), plan
    assert ("act: one launch" in plan) != ("+ select kernel" in plan), plan
    r = set()
    for flag, text in (("chains", "grl plan: q chains"), ("chained", "inside the backward chains"), ("apply", "in one launch: yes"),
                       ("q_pf", "grl plan: q_pf "), ("act", "act: one launch")):
        if text in plan:
            r.add(flag)
    if matrix_cores:
        assert "chains" not in r or ("matrix-core stages" in plan) != ("VALU stages" in plan), plan
        if "matrix-core stages" in plan:
            r.add("mfma")
            if "grl plan: q_l0" not in plan:
                r.add("l0")
    return frozenset(r)


def make_q_case(algo, obs_dim, D, bins, common, branch, value, B, n_replay=40, n_steps=3, seed=0, lr=1e-3,
                normalize=False, loss_sum=False, trunk_rescale=True, uniform=False):
    rng = np.random.default_rng(seed)
    spec = od.QSpec(algo=algo, obs_dim=obs_dim, n_branches=D, n_bins=bins, common=list(common),
                    branch_hidden=list(branch), value_hidden=list(value), gamma=0.97, lr=lr,
                    loss_sum_branches=loss_sum, trunk_rescale=trunk_rescale)
    cfg = _capi.make_q_config(algo, obs_dim, D, bins, common, branch, value, batch_size=B, act_batch=4,
                              replay_capacity=n_replay, gamma=0.97, lr=lr, normalize=normalize,
                              loss_sum_branches=loss_sum, trunk_rescale=trunk_rescale)
    mean, var = rng.uniform(0.2, 0.8, obs_dim), rng.uniform(0.05, 0.2, obs_dim)
    tr = {"obs": rng.normal(mean, np.sqrt(var), (n_replay, obs_dim)).astype(np.float32),
          "next_obs": rng.normal(mean, np.sqrt(var), (n_replay, obs_dim)).astype(np.float32),
          "act": rng.integers(0, bins, (n_replay, D)).astype(np.float32),
          "rew": rng.normal(0, 2.0, n_replay).astype(np.float32),
          "done": (rng.random(n_replay) < 0.2).astype(np.float32)}
    idx = rng.integers(0, n_replay, (n_steps, B), dtype=np.int64)
    weights = rng.uniform(0.3, 1.0, (n_steps, B)).astype(np.float32)
    if uniform:                   # uniform replay (prioritized_replay False): stable-baselines feeds weights of one
        weights = np.ones((n_steps, B), np.float32)
    return dict(spec=spec, cfg=cfg, tr=tr, idx=idx, weights=weights, params=od.init_params(spec, seed), B=B,
                n_steps=n_steps, stats={"mean": mean, "var": var, "ret_var": 9.0}, normalize=normalize)


TIE_REL = 1e-4          # the project's forward tolerance (run_and_compare): closer top-two Q-values are not compared
TIE_CAP = 0.05          # ... for at most this share of the (row, branch) pairs of a case


def compared_pairs(q):
    """[n, D] mask of the (row, branch) pairs whose two largest oracle Q-values differ by more than the forward tolerance."""
    top = np.sort(q, axis=2)[:, :, -2:]
    return (top[:, :, 1] - top[:, :, 0]) > TIE_REL * np.maximum(np.abs(top[:, :, 1]), np.abs(top[:, :, 0]))


ACT_NS = (1, 16, 17, 64)          # one row; one full row block; a second, ragged one; four


def act_case(name, n):
    """A SHAPE_CASES network for the act path: seeded Xavier weights, biases away from zero (the value tower and every bias add
    take part), n standard-normal observations, act_batch n.  With these seeds the oracle alone leaves at most two pairs of any
    (case, n) out as ties (tests/test_gpu_q_act.py::test_tie_cap_holds_for_the_oracle_alone asserts the cap for every one)."""
    a = case_args(name)
    spec = od.QSpec(algo=a["algo"], obs_dim=a["obs_dim"], n_branches=a["D"], n_bins=a["bins"], common=list(a["common"]),
                    branch_hidden=list(a["branch"]), value_hidden=list(a["value"]))
    params = od.init_params(spec, seed=11)
    rng = np.random.default_rng(12)
    for k in params:
        if k.endswith("biases:0"):
            params[k] = rng.uniform(-0.1, 0.1, params[k].shape).astype(np.float32)
    cfg = _capi.make_q_config(spec.algo, spec.obs_dim, spec.n_branches, spec.n_bins, tuple(spec.common), tuple(spec.branch_hidden),
                              tuple(spec.value_hidden), batch_size=8, act_batch=n, replay_capacity=16)
    obs = np.random.default_rng(100 + n).normal(0.0, 1.0, (n, spec.obs_dim)).astype(np.float32)
    return spec, params, cfg, obs


def act_bins_check(name, n, read_plan, backend=None, lib_path=None):
    """grl_act(GRL_ACT_GREEDY) of a SHAPE_CASES network on n rows against the arg-max of the oracle (the body of
    tests/test_gpu_q_act.py::test_bins_equal_the_argmax_of_the_oracle) on the route the case declares, plus the override
    table on the first row block.  read_plan() returns the GRL_PLAN_DUMP text written since the last call."""
    spec, params, cfg, obs = act_case(name, n)
    fused = "act" in declared_route(name)
    q = od.QOracle(spec, params).q_values(obs)
    keep = compared_pairs(q)
    assert keep.any() and (~keep).mean() <= TIE_CAP, (~keep).mean()
    eng = QEngine(cfg, backend=backend, lib_path=lib_path)
    try:
        plan = read_plan()
        assert ("epsilon-greedy act: one launch" in plan) == fused and ("+ select kernel" in plan) != fused, plan
        eng.set_parameters(params)
        bins = eng.act_bins(obs)
        assert bins.shape == (n, spec.n_branches) and bins.dtype == np.int64
        want = q.argmax(axis=2)
        print("%s n=%d (%s): %d of %d pairs compared, %d left out as ties, %d differ" % (
            name, n, "one launch" if fused else "select kernel", keep.sum(), keep.size, (~keep).sum(), (bins != want)[keep].sum()))
        assert np.array_equal(bins[keep], want[keep])
        assert np.array_equal(eng.act_bins(obs[:1]), bins[:1])                  # fewer rows than act_batch
        assert np.array_equal(eng.act_bins(obs), bins)                           # and again: the completion counter keeps step
        qd = eng.q_values(obs)
        assert np.array_equal(qd.argmax(axis=2)[keep], want[keep])
        assert np.array_equal(eng.q_values(obs), qd)
        m, D = min(n, 16), spec.n_branches                                      # the override table on one row block
        rng = np.random.default_rng(1)
        explore = np.where(rng.random((m, D)) < 0.5, rng.integers(0, spec.n_bins, (m, D)), -1)
        explore[0] = -1                                                         # an all-greedy row
        explore[m - 1] = np.arange(D) % spec.n_bins                             # an all-explored row (the only row when n == 1)
        assert np.array_equal(eng.act_bins(obs[:m], explore), np.where(explore >= 0, explore, bins[:m]))
        assert np.array_equal(eng.act_bins(obs), bins)
    finally:
        eng.close()


def nan_branch_check(name, read_plan, n=17, backend=None, lib_path=None):
    """One output bias of ONE branch NaN: the dueling mean carries it to every Q-value of that branch, and the arg-max of an
    all-NaN row is bin 0 (np.argmax; csrc/q_act.h qa_better) -- on the route the case declares.  The other branches keep the
    greedy bins of the clean network."""
    spec, params, cfg, obs = act_case(name, n)
    D, nb = spec.n_branches, spec.n_bins
    assert D >= 2
    fused = "act" in declared_route(name)
    keep = compared_pairs(od.QOracle(spec, params).q_values(obs))
    want = od.QOracle(spec, params).q_values(obs).argmax(axis=2)
    outs = [k for k in params if "/target_q_func/" not in k and "/action_value/" in k and k.endswith("weights:0")
            and params[k].shape[1] == nb]
    kb = outs[len(outs) // 2].replace("weights:0", "biases:0")
    bad = dict(params)
    bad[kb] = np.array(params[kb])
    bad[kb][nb // 2] = np.nan
    eng = QEngine(cfg, backend=backend, lib_path=lib_path)
    try:
        assert ("epsilon-greedy act: one launch" in read_plan()) == fused
        eng.set_parameters(bad)
        bins, qd = eng.act_bins(obs), eng.q_values(obs)
        nan_branch = np.isnan(qd).all(axis=(0, 2))
        assert nan_branch.sum() == 1 and not np.isnan(qd[:, ~nan_branch]).any(), np.isnan(qd).mean(axis=(0, 2))
        assert np.array_equal(bins[:, nan_branch], np.zeros((n, 1), np.int64)), bins[:, nan_branch].ravel()
        assert np.array_equal(bins[:, nan_branch], qd.argmax(axis=2)[:, nan_branch])
        rest = keep & ~nan_branch[None, :]
        assert rest.any() and np.array_equal(bins[rest], want[rest]) and np.array_equal(bins[rest], qd.argmax(axis=2)[rest])
        print("%s (%s): branch %d all NaN -> bin 0 on %d rows; %d other pairs keep their greedy bins" % (
            name, "one launch" if fused else "select kernel", int(np.argmax(nan_branch)), n, rest.sum()))
    finally:
        eng.close()


def value_chain_check(name, read_plan, n=17, backend=None, lib_path=None):
    """The greedy bins do not depend on a finite state value (it is added to every bin of a branch), so a value chain of
    q_act_kernel that read the wrong activations would pass every arg-max comparison.  Here it would not: unit 0 of every hidden
    layer of the value tower is dead (bias -1e6: its activation is exactly 0) and its outgoing weights are 1e30, while unit 0 of
    every trunk and branch layer is strongly alive (bias +50).  Read from the value tower's own buffer the poisoned weights meet
    zeros and the bins are those of the oracle; read from anywhere else the state value reaches ~1e31, absorbs every advantage,
    and all bins of the row tie at bin 0."""
    spec, params, cfg, obs = act_case(name, n)
    sc = spec.scope + "/model/"
    idx = lambda k: int(k.split("fully_connected")[1].split("/")[0].lstrip("_") or 0)
    p = {k: np.array(v) for k, v in params.items()}
    value_w = sorted((k for k in p if k.startswith(sc + "state_value/") and k.endswith("weights:0")), key=idx)
    assert len(value_w) == len(spec.value_hidden) + 1
    for below, above in zip(value_w[:-1], value_w[1:]):
        p[below.replace("weights:0", "biases:0")][0] = -1e6
        p[above][0, :] = 1e30
    n_branch_hidden = len(spec.branch_hidden)
    for k in p:
        if not k.startswith(sc) or not k.endswith("biases:0") or "/state_value/" in k:
            continue
        if "/action_value/" in k and idx(k) % (n_branch_hidden + 1) == n_branch_hidden:
            continue                                    # a branch's output layer
        p[k][0] = 50.0
    q = od.QOracle(spec, p).q_values(obs)
    assert np.isfinite(q).all() and np.abs(q).max() < 1e4
    keep = compared_pairs(q)
    want = q.argmax(axis=2)
    assert (~keep).mean() <= TIE_CAP and (want[keep] != 0).sum() >= keep.sum() // 4     # bin 0 is not the answer anyway
    eng = QEngine(cfg, backend=backend, lib_path=lib_path)
    try:
        assert "epsilon-greedy act: one launch" in read_plan()
        eng.set_parameters(p)
        bins = eng.act_bins(obs)
        print("%s: value tower poisoned behind dead units: %d of %d pairs compared, %d differ" % (
            name, keep.sum(), keep.size, (bins != want)[keep].sum()))
        assert np.array_equal(bins[keep], want[keep])
        pu.close(eng.q_values(obs), q, atol=2e-5, rtol=2e-4, what="Q-values with the poisoned value tower")
    finally:
        eng.close()


def shipped_big_trained_case(golden_dir):
    """SHAPE_CASES["shipped_big"] as the reference left it: the weights of trained_models/BDQ_33pads_big/best_model as starting
    parameters and its two real auto-encoder feature vectors among the replay rows, drawn in every minibatch."""
    import os
    case = make_q_case(**case_args("shipped_big"))
    z = np.load(os.path.join(golden_dir, "bdq_33_big_best_model.npz"))
    assert set(z.files) == set(case["params"])
    case["params"] = {k: z[k] for k in z.files}
    real = np.load(os.path.join(golden_dir, "vecnorm_encoder.npz"))["real_obs"][:, :case["spec"].obs_dim].astype(np.float32)
    case["tr"]["obs"][:2] = real
    case["tr"]["next_obs"][0] = real[1]
    case["idx"][:, 0], case["idx"][:, 1] = 0, 1
    return case


def q_engine_setup(case, backend=None, lib_path=None):
    eng = QEngine(case["cfg"], backend=backend, lib_path=lib_path)
    eng.set_parameters(case["params"])
    st = case["stats"]
    eng.set_obs_stats(st["mean"], st["var"], st["ret_var"])
    tr = case["tr"]
    eng.replay_add(tr["obs"], tr["act"], tr["rew"], tr["next_obs"], tr["done"])
    return eng


def _batch(case, s):
    from oracle import sac as osac
    tr, ii = case["tr"], case["idx"][s]
    obs, nxt, rew = tr["obs"][ii], tr["next_obs"][ii], tr["rew"][ii]
    if case["normalize"]:
        st = case["stats"]
        obs = osac.normalize_obs(obs, st["mean"], st["var"])
        nxt = osac.normalize_obs(nxt, st["mean"], st["var"])
        rew = osac.normalize_reward(rew, st["ret_var"])
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    return {"obs": f(obs), "next_obs": f(nxt), "act": f(tr["act"][ii]), "rew": f(rew), "done": f(tr["done"][ii])}


def run_and_compare(case, backend=None, lib_path=None):
    spec = case["spec"]
    orc = od.QOracle(spec, case["params"])
    eng = q_engine_setup(case, backend, lib_path)
    B, D = case["B"], spec.n_branches
    # act path
    obs4 = case["tr"]["obs"][:3]
    pu.close(eng.q_values(obs4), orc.q_values(obs4), atol=2e-5, rtol=2e-4, what="Q-values (act path)")
    for s in range(case["n_steps"]):
        ref = orc.step(_batch(case, s), case["weights"][s])
        eng.compute_grads(case["idx"][s:s + 1], case["weights"][s:s + 1])
        pu.close(eng.td_errors(), ref["td"], atol=3e-5, rtol=2e-4, what="td step %d" % s)
        pu.close(eng.priorities(), ref["priority"], atol=1e-4, rtol=2e-4, what="priority")
        if s == 0:
            G = eng.get_gradients()
            for n, g in ref["grads"].items():
                pu.close_rel_max(G[n], g, what="grad " + n)
            assert abs(eng.metrics()["policy_loss"] - ref["loss"]) <= 1e-4 * abs(ref["loss"]) + 1e-6
        eng.apply_grads(1.0)
        if s == 1:
            eng.update_target()
            orc.update_target()
    pu.compare_params(eng, orc, spec.lr, case["n_steps"])
    P = eng.get_parameters()
    sc = spec.scope
    for n in P:                                             # hard copy happened after step 1 only
        if "/target_q_func/" in n:
            assert not np.array_equal(P[n], P[n.replace("/target_q_func", "")]) or P[n].size <= 1, n
    assert P[sc + "/eps:0"] == case["params"][sc + "/eps:0"]
    # fused call == split calls
    eng2 = q_engine_setup(case, backend, lib_path)
    eng2.train(2, case["idx"][:2], case["weights"][:2])
    eng3 = q_engine_setup(case, backend, lib_path)
    for s in range(2):
        eng3.compute_grads(case["idx"][s:s + 1], case["weights"][s:s + 1])
        eng3.apply_grads(1.0)
    Pa, Pb = eng2.get_parameters(), eng3.get_parameters()
    for n in Pa:
        assert np.array_equal(Pa[n], Pb[n]), n
    for e in (eng, eng2, eng3):
        e.close()


# ---------------------------------------------------------------------------------------------------
# prioritised replay on the device (csrc/per_kernels.h) against oracle/per.py, draw for draw
def _leaves_equal(dev, ref, exact, what):
    """float64 leaves: bit-equal; `exact=False` (GPU, leaves written by `add` after max_priority left 1.0) allows the
    last bit of a FLOAT64 pow to differ between the device's math library and libm."""
    if exact:
        assert np.array_equal(dev, ref), "%s: %d leaves differ, max rel %.3e" % (
            what, int((dev != ref).sum()), float(np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300))))
    else:
        assert np.all(np.abs(dev - ref) <= np.spacing(np.abs(ref))), what


def per_check(backend=None, lib_path=None, cap=3000, n_store=2500, B=16, n_steps=5, seed=3, case_name="dqn",
              stratified=False):
    """Fill, then alternate (sample with explicit float64 uniforms -> update -> leaves written back) for n_steps
    rounds, then add across the ring wrap and sample again.  The oracle (stable-baselines' segment trees, restated in
    oracle/per.py) and the device evolve INDEPENDENTLY: the only values handed from one to the other are the
    uniforms and, as in DQN.learn, the TD errors of the minibatch.  After every round the drawn indices must be
    EQUAL and the float64 leaves bit-identical; the importance weights agree to float32 rounding."""
    from oracle.per import PerOracle
    rng = np.random.default_rng(seed)
    c = dict(CASES[case_name])
    c["B"] = B
    case = make_q_case(n_replay=n_store, n_steps=n_steps, **c)
    case["cfg"].replay_capacity = cap
    case["cfg"].q_per, case["cfg"].q_per_alpha, case["cfg"].q_per_eps = 1, 0.6, 1e-6
    case["cfg"].q_per_alpha64, case["cfg"].q_per_stratified = 0.6, int(stratified)
    eng = q_engine_setup(case, backend=backend, lib_path=lib_path)
    on_cpu = backend is not None
    orc = PerOracle(cap, 0.6, 1e-6, stratified=stratified)
    orc.add(n_store)
    p0 = eng.stored_priorities()
    assert p0.dtype == np.float64 and np.array_equal(p0, orc.leaves) and not p0[n_store:].any()

    def one_round(s, beta):
        u = rng.random(B)                               # float64, like np.random.random
        eng.train_per(1, beta, u[None])
        idx = eng.sampled_indices()
        ref_idx, ref_w = orc.sample(u, beta)
        assert np.array_equal(idx, ref_idx), (s, idx, ref_idx)
        assert idx.max() <= orc.size - 2                # the published sum(0, len - 1) never draws the newest transition
        w = eng.importance_weights()
        assert np.allclose(w, ref_w.astype(np.float32), rtol=1e-6, atol=0), (w, ref_w)
        assert w.max() <= 1.0 + 1e-6 and w.min() > 0
        orc.update(idx, eng.priorities())               # |td| of the minibatch just trained on (sum over branches)
        return idx

    for s in range(n_steps):
        one_round(s, 0.4 + 0.1 * s)
        _leaves_equal(eng.stored_priorities(), orc.leaves, True, "leaves after update %d" % s)
    assert float(orc._max_priority) > 1.0              # the TD errors of these cases exceed 1: `add` now takes a float64 power
    # new transitions enter with max_priority ** alpha, ring wrap included; then sampling goes on over the mixed leaves
    tr = case["tr"]
    k = cap - n_store + 7
    eng.replay_add(tr["obs"][:k], tr["act"][:k], tr["rew"][:k], tr["next_obs"][:k], tr["done"][:k])
    orc.add(k)
    _leaves_equal(eng.stored_priorities(), orc.leaves, on_cpu, "leaves after add")
    if on_cpu:
        for s in range(2):
            one_round(n_steps + s, 0.9 + 0.05 * s)
            _leaves_equal(eng.stored_priorities(), orc.leaves, True, "leaves after update %d" % (n_steps + s))
    # device RNG path: runs, indices in range
    eng.train_per(2, 1.0)
    idx = eng.sampled_indices()
    assert idx.min() >= 0 and idx.max() < cap
    tot = float(orc._it_sum.sum())
    eng.close()
    return tot


def uniform_multi_update_check(monkeypatch, name, n_store, backend=None, lib_path=None, n=7):
    """Uniform replay on the device RNG (what gripper_grasp.yaml:106 selects for BDQ): ONE call of n updates -- the index draw and
    the gather of update t + 1 ride on the apply launch of update t, the forward launch opens each update (plan_q "q_pf", four
    launches per update) -- == n calls of one update == the same with GRL_TUNE q_pf=0: parameters, Adam moments, the last drawn
    indices and the metrics bit for bit."""
    def run(split, env=None):
        if env:
            monkeypatch.setenv("GRL_TUNE", env)
        case = make_q_case(**case_args(name, n_replay=n_store, n_steps=1))
        eng = q_engine_setup(case, backend, lib_path)
        for k in split:
            eng.train_device(k)
        out = (eng.get_parameters(), eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy(), eng.sampled_indices(), eng.metrics())
        eng.close()
        if env:
            monkeypatch.delenv("GRL_TUNE")
        return out
    ref = run([1] * n)
    for got in (run([n]), run([2, n - 2]), run([n - 3, 1, 2]), run([n], env="q_pf=0")):
        for k in ref[0]:
            assert np.array_equal(ref[0][k], got[0][k]), k
        assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])
        assert np.array_equal(ref[3], got[3]) and ref[4] == got[4]


def per_multi_update_check(monkeypatch, name, cap, n_store, backend=None, lib_path=None, n=9):
    """Prioritised replay on the device RNG: ONE call of n updates (the first sums every block of the ring, every apply
    launch rebuilds the blocks its priority write-back touched, the later samplers start from those -- per_refresh_body) ==
    n calls of one update (a block-sum pass over the whole ring in front of every sampler) == the same with GRL_TUNE
    per_inc=0: drawn indices, float64 leaves and parameters bit for bit.  (Several samples per 1024-leaf block, repeated
    indices, the block that holds leaf size - 2.)"""
    def run(split, env=None):
        if env:
            monkeypatch.setenv("GRL_TUNE", env)
        case = make_q_case(**case_args(name, n_replay=n_store, n_steps=1))
        case["cfg"].replay_capacity = cap
        case["cfg"].q_per, case["cfg"].q_per_alpha, case["cfg"].q_per_eps = 1, 0.6, 1e-6
        case["cfg"].q_per_alpha64 = 0.6
        eng = q_engine_setup(case, backend, lib_path)
        idx = []
        for k in split:
            eng.train_per(k, 0.7)
            idx.append(eng.sampled_indices())
        out = (eng.get_parameters(), eng.stored_priorities(), idx[-1], eng.metrics())
        eng.close()
        if env:
            monkeypatch.delenv("GRL_TUNE")
        return out
    ref = run([1] * n)
    assert np.count_nonzero(ref[1] != ref[1][0]) > min(100, n * 4)            # the priorities moved
    splits = ([n], [2, n - 2], [n - 4, 1, 3])
    for got in [run(list(sp)) for sp in splits] + [run([n], env="per_inc=0")]:
        for k in ref[0]:
            assert np.array_equal(ref[0][k], got[0][k]), k
        assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2]) and ref[3] == got[3]
