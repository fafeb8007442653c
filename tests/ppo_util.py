"""PPO2 on the engine (csrc/plan_ppo.inl, csrc/ppo_kernels.h) against a float64 restatement of the update.

Nothing in the reference pins PPO (no zip, log or test ships with it), and oracle/ knows no PPO, so stable-baselines 2.10.1
`ppo2.py` / `common/policies.py` / `common/distributions.py` are restated here in torch float64 with autograd: the two tanh
towers, the diagonal Gaussian, the clipped surrogate and the clipped value loss with TF's `maximum` rule spelled out
(`torch.where(x >= y, x, y)`: the gradient goes to x where x >= y), the advantage normalisation with the population standard
deviation, clip_by_global_norm and TF-Adam with epsilon 1e-5.  GAE is restated in NumPy float32 in the operation order the
kernel is held to, bit for bit.  The same helpers drive a handle of the emulation build (tests/test_hostemu_ppo.py) and of the
device (tests/test_gpu_ppo.py), as q_parity_util.py does.

Tolerances are the project's: forward |d| <= 1e-5 + 1e-4 |ref|; every gradient tensor within 1e-3 max|g|;
parameters after n updates on the scale of the update, max |d| <= 0.3 lr n and mean |d| <= 0.02 lr n per tensor
(parity_util.compare_params).  A row within MARGIN of a branch boundary of the loss (ratio at 1 +- c, |v - old_v| at c_v,
the two arguments of a maximum equal) could take the other branch in float32: `Ref.update` reports the smallest such distance of
every minibatch and the tests assert, on the reference alone and before anything is compared, that none is that close."""
from collections import OrderedDict

import numpy as np
import torch

from grasp_rl import _capi
from grasp_rl.engine import PpoEngine

MARGIN = 1e-5
LOG_2PI = float(np.log(2.0 * np.pi))

# shape -> arguments of make_case.  Small on purpose: odd sizes, rows that are no multiple of a tile, towers that differ, more than
# one block of the loss launch, and each route of the plan (one-launch act / launch list; first layer whole / in partial sums)
CASES = {
    "default_64_64": dict(obs_dim=101, A=5, n_envs=2, n_steps=16, nmb=4, pi=(64, 64), vf=(64, 64)),
    "odd_towers": dict(obs_dim=13, A=3, n_envs=3, n_steps=7, nmb=3, pi=(24,), vf=(40, 17, 9)),
    "two_blocks": dict(obs_dim=20, A=2, n_envs=4, n_steps=75, nmb=1, pi=(16, 16), vf=(16,)),               # 300 rows: two loss blocks
    "wide_obs": dict(obs_dim=2310, A=5, n_envs=2, n_steps=8, nmb=2, pi=(64, 64), vf=(64, 64)),             # beyond 2048: split-K layer 0, launch list
    "width_300": dict(obs_dim=30, A=4, n_envs=2, n_steps=6, nmb=2, pi=(300, 20), vf=(12,)),                # a width beyond 256: launch list
    "no_vf_clip": dict(obs_dim=11, A=1, n_envs=1, n_steps=12, nmb=2, pi=(8, 8), vf=(8, 8), cliprange_vf=-1.0, max_grad_norm=None),
}


# ---------------------------------------------------------------------------------------------------
# Shapes ON the edges of what csrc/plan_ppo.inl and csrc/ppo_kernels.h decide by shape alone (tests/test_gpu_ppo_shapes.py on the
# MI355X, tests/test_hostemu_ppo_shapes.py on the emulation build), the smallest that still cross each edge.  `route` is what the
# case exists for, written down from the conditions in the sources (restated in planned_route below), never from what the engine
# prints:
#   one | list_obs | list_width   the act path: ppo_act_kernel, or the launch list because of the observation / because of a width
#   whole | split                 the first layer of the towers: one product, or partial sums that tanh_fwd adds (any call, any tower)
#   quads | scalars               tanh_fwd over partial sums: 16-byte accesses, or none at all (`part_stride & 3`)
#   straddle                      ... quads with H % 4 != 0: a float4 runs over a row end, the bias index wraps inside it
#   grid2                         a first-level tanh launch beyond 1024 x 256 quads: the grid-stride loops take a second pass
# The stride of the partial sums IS rows * H (engine.hip: set_split), so `part_stride % 4 == 0` together with `rows * H % 4 != 0`
# -- quads AND a scalar tail over partial sums -- cannot be planned: no `wide_tail` case; route_from_dump asserts the two numbers of
# every dumped line equal, so a stride that stops being rows * H fails here first.  What is no route of the plan sits in the
# comments: loss blocks of 256 rows, GAE blocks of 64 environments, the 256-lane loops of the rewards and the gather statistics.
# Every case passes check_update's preconditions at seed 0 except grid_stride (seeds 0 and 1 put a row within 1e-5 of a boundary)
# and envs_257 (seed 0 passes with a margin of 1.7e-5 only; seed 7 leaves 3.0e-4, the most of seeds 0 ... 9).
SHAPE_CASES = {
    # one launch AT the input limit: the staging loop of ppo_act_kernel takes 8 passes
    "act_in_2048": dict(obs_dim=2048, A=2, n_envs=2, n_steps=4, nmb=1, pi=(8,), vf=(8,), route="one whole"),
    # one value beyond: launch list, split first layer; 1 x 17, 1 x 9, 7 x 17 and 7 x 9 floats per part: no quads, all scalars
    "in_2049_odd": dict(obs_dim=2049, A=3, n_envs=1, n_steps=7, nmb=1, pi=(17,), vf=(9, 5), route="list_obs split scalars"),
    # H % 4 != 0 with rows * H % 4 == 0 (2 x 6, 2 x 10, 6 x 6, 6 x 10): quads that straddle rows
    "wide_quads": dict(obs_dim=2052, A=2, n_envs=2, n_steps=3, nmb=1, pi=(6,), vf=(10,), route="list_obs split quads straddle"),
    # (added) ... and with H odd, rows a multiple of 4 (4 x 5, 4 x 7, 8 x 5, 8 x 7).  A quad starts at a multiple of 4, so with H even
    # only its third and fourth component ever cross a row end; with H = 5 and 7 each of the last three does
    "wide_quads_odd": dict(obs_dim=2052, A=2, n_envs=4, n_steps=2, nmb=1, pi=(5,), vf=(7,), route="list_obs split quads straddle"),
    # one launch AT the width limit: Np = 256, S = 1 (256, 255), Np = 256 over 129 live outputs; staging loop 2 passes
    "width_256": dict(obs_dim=300, A=2, n_envs=2, n_steps=5, nmb=1, pi=(256,), vf=(255, 129), route="one whole"),
    "width_257": dict(obs_dim=300, A=2, n_envs=2, n_steps=5, nmb=1, pi=(257,), vf=(8,), route="list_width whole"),
    # GRL_MAX_LAYERS: the hs[l & 1] ping-pong goes round twice; towers of depth 4 and 1
    "depth_4_1": dict(obs_dim=9, A=2, n_envs=2, n_steps=9, nmb=2, pi=(8, 7, 6, 5), vf=(3,), route="one whole"),
    # PPO_MAX_A: the closing sum of the loss crosses a wave, ws[..] to its last column, the gather's t == 64 lane, the sample tail
    "A_64": dict(obs_dim=10, A=64, n_envs=2, n_steps=10, nmb=2, pi=(16,), vf=(16,), route="one whole"),
    "envs_65": dict(obs_dim=6, A=2, n_envs=65, n_steps=2, nmb=1, pi=(8,), vf=(8,), route="one whole"),       # two GAE workgroups
    # rewards loop second pass, n_steps = 1 (every step is the `end` step), 257 rows: a loss block with ONE live row, the gather's
    # statistics in two passes
    "envs_257": dict(obs_dim=6, A=2, n_envs=257, n_steps=1, nmb=1, pi=(8,), vf=(8,), route="one whole", seed=7),
    "mb_256": dict(obs_dim=6, A=2, n_envs=4, n_steps=128, nmb=2, pi=(8,), vf=(8,), route="one whole"),       # exactly one full loss block
    "mb_512": dict(obs_dim=6, A=2, n_envs=4, n_steps=128, nmb=1, pi=(8,), vf=(8,), route="one whole"),       # exactly two
    # 4100 x 257 floats: 263 425 quads against 1024 x 256, so tanh_fwd / tanh_bwd take a second pass (and a scalar tail of one)
    "grid_stride": dict(obs_dim=4, A=2, n_envs=1, n_steps=4100, nmb=1, pi=(257,), vf=(4,), route="list_width whole grid2", seed=2),
}
ACT_SHAPE_CASES = ("act_in_2048", "in_2049_odd", "wide_quads_odd", "width_256", "width_257", "depth_4_1", "A_64", "envs_65", "envs_257")
ONE_LAUNCH_VS_LIST = ("act_in_2048", "width_256", "A_64")


def case_args(name):
    a = dict(CASES[name] if name in CASES else SHAPE_CASES[name])
    a.pop("route", None)
    return a


def declared_route(name, table=None):
    return frozenset((SHAPE_CASES if table is None else table)[name]["route"].split())


def first_layer_calls(a):
    """(rows, widths of the first layers planned together) of every PpoPlanner::forward call of a PPO2 handle."""
    both = (a["pi"][0], a["vf"][0])
    one_launch = a["obs_dim"] <= 2048 and max(tuple(a["pi"]) + tuple(a["vf"])) <= 256      # (no forward call on the act path then)
    return ([] if one_launch else [(a["n_envs"], both)]) + [(a["n_envs"] * a["n_steps"] // a["nmb"], both)]


def planned_route(obs_dim, widths, calls):
    """The conditions of csrc/plan_ppo.inl (routes, forward), engine.hip (set_split), csrc/ppo_kernels.h (tanh_fwd_kernel) and
    csrc/ppo.hip (tanh_grid) with no GRL_TUNE switch set, restated: PPO_ACT_MAX_IN 2048, PPO_ACT_MAX_HID 256, a reduction cut until
    the launch has 64 tiles of 64 x 64 in chunks of whole 32-value steps, 1024 workgroups of 256 quads."""
    r = set()
    r.add("list_obs" if obs_dim > 2048 else ("list_width" if max(widths) > 256 else "one"))
    cdiv = lambda x, y: (x + y - 1) // y
    for rows, hs in calls:
        for H in hs:
            split = 1
            if obs_dim > 2048:
                base = len(hs) * cdiv(rows, 64) * cdiv(H, 64)
                steps = cdiv(obs_dim, 32)
                per = cdiv(steps, max(1, min(cdiv(64, base), steps)))
                split = cdiv(obs_dim, per * 32)
            r.add("split" if split > 1 else "whole")
            if split > 1:
                part_stride = rows * H
                r.add("scalars" if part_stride % 4 else "quads")
                if part_stride % 4 == 0 and H % 4:
                    r.add("straddle")
        if cdiv(rows * max(hs), 4) > 1024 * 256:
            r.add("grid2")
    return frozenset(r)


def route_from_dump(plan):
    """The route a GRL_PLAN_DUMP=1 text of a PPO2 / TRPO handle reports (lines `grl plan: ppo_act` and `grl plan: ppo_l0`)."""
    import re
    act = sorted(set(l for l in plan.splitlines() if l.startswith("grl plan: ppo_act ")))      # (sizing and creation both plan)
    assert len(act) == 1, plan
    r = set()
    if "one launch per call" in act[0]:
        r.add("one")
    else:
        assert "launch list (" in act[0], act
        r.add("list_obs" if "observation beyond 2048 values" in act[0] else "list_width")
        assert ("observation beyond 2048 values" in act[0]) != ("a width beyond 256" in act[0]), act
    l0 = [l for l in plan.splitlines() if l.startswith("grl plan: ppo_l0 ")]
    assert l0, plan
    for line in l0:
        rows = int(re.search(r": (\d+) rows;", line).group(1))
        towers = re.findall(r"(pi|vf) H (\d+) (whole|split \d+) \(([^)]*)\)", line)
        assert towers, line
        for _, H, how, detail in towers:
            H = int(H)
            tail = int(re.search(r"rows \* H % 4 = (\d)", detail).group(1))
            assert tail == rows * H % 4, line
            if how == "whole":
                r.add("whole")
                continue
            assert int(how.split()[1]) > 1, line
            stride4 = int(re.search(r"part_stride % 4 = (\d)", detail).group(1))
            assert stride4 == tail, "the stride of the partial sums is no longer rows * H: " + line
            r.add("split")
            r.add("scalars" if stride4 else "quads")
            if not stride4 and H % 4:
                r.add("straddle")
        if (rows * max(int(t[1]) for t in towers) + 3) // 4 > 1024 * 256:
            r.add("grid2")
    return frozenset(r)


def tower_shapes(case):
    return tuple(case["pi"]), tuple(case["vf"])


def param_names(pi, vf):
    """TF creation order: layer index outermost, pi before vf, a tower that has run out of layers skipped; then vf, pi, logstd, q."""
    out = []
    for l in range(max(len(pi), len(vf))):
        for nm, t in (("pi", pi), ("vf", vf)):
            if l < len(t):
                out += ["model/%s_fc%d/w:0" % (nm, l), "model/%s_fc%d/b:0" % (nm, l)]
    return out + ["model/vf/w:0", "model/vf/b:0", "model/pi/w:0", "model/pi/b:0", "model/pi/logstd:0", "model/q/w:0", "model/q/b:0"]


def param_shapes(obs_dim, A, pi, vf):
    sh = OrderedDict()
    for n in param_names(pi, vf):
        scope = n.split("/")[1]
        if "_fc" in scope:
            t = pi if scope.startswith("pi") else vf
            l = int(scope.split("_fc")[1])
            k = obs_dim if l == 0 else t[l - 1]
            sh[n] = (k, t[l]) if n.endswith("w:0") else (t[l],)
        elif scope == "vf":
            sh[n] = (vf[-1], 1) if n.endswith("w:0") else (1,)
        elif scope == "pi":
            sh[n] = (pi[-1], A) if n.endswith("/w:0") else ((A,) if n.endswith("/b:0") else (1, A))
        else:
            sh[n] = (vf[-1], A) if n.endswith("w:0") else (A,)
    return sh


def _ortho(shape, scale, rng):
    u, _, vt = np.linalg.svd(rng.normal(0.0, 1.0, shape), full_matrices=False)
    return (scale * (u if u.shape == shape else vt)).astype(np.float32)


def init_params(obs_dim, A, pi, vf, seed, everything_takes_part=True):
    """Orthogonal weights with stable-baselines' gains; with `everything_takes_part` biases and logstd away from zero and a policy
    output layer large enough for the means to matter (gain 0.5 instead of 0.01)."""
    rng = np.random.default_rng(seed)
    P = OrderedDict()
    for n, shp in param_shapes(obs_dim, A, pi, vf).items():
        if n.endswith("/w:0"):
            gain = {"model/pi/w:0": 0.5 if everything_takes_part else 0.01, "model/q/w:0": 0.01, "model/vf/w:0": 1.0}.get(n, np.sqrt(2.0))
            P[n] = _ortho(shp, gain, rng)
        elif everything_takes_part:
            P[n] = rng.uniform(-0.3, 0.3, shp).astype(np.float32)
        else:
            P[n] = np.zeros(shp, np.float32)
    return P


# ------------------------------------------------------------------------------------------------- GAE, NumPy float32
def gae_np(rew, val, done, last_v, last_done, gamma, lam):
    """rew / val / done [n_envs, n_steps] float32 (done: the flags from BEFORE each step), last_v / last_done [n_envs].
    Every operation rounded to float32, in the order the kernel is held to."""
    f = np.float32
    rew, val, done = (np.asarray(a, f) for a in (rew, val, done))
    last_v, last_done = np.asarray(last_v, f), np.asarray(last_done, f)
    n_envs, T = rew.shape
    g, c = f(gamma), f(float(gamma) * float(lam))
    adv = np.zeros((n_envs, T), f)
    last = np.zeros(n_envs, f)
    for t in range(T - 1, -1, -1):
        nnt = f(1.0) - (last_done if t == T - 1 else done[:, t + 1])
        nv = last_v if t == T - 1 else val[:, t + 1]
        delta = ((g * nv) * nnt + rew[:, t]) - val[:, t]
        last = ((c * nnt) * last) + delta
        adv[:, t] = last
    return adv, adv + val


# ------------------------------------------------------------------------------------------------- float64 restatement
def forward64(T, obs, pi, vf):
    def tower(nm, widths):
        h = obs
        for l in range(len(widths)):
            h = torch.tanh(h @ T["model/%s_fc%d/w:0" % (nm, l)] + T["model/%s_fc%d/b:0" % (nm, l)])
        return h
    mean = tower("pi", pi) @ T["model/pi/w:0"] + T["model/pi/b:0"]
    v = (tower("vf", vf) @ T["model/vf/w:0"] + T["model/vf/b:0"])[:, 0]
    return mean, v


def neglogp64(a, mean, logstd):
    return 0.5 * (((a - mean) / torch.exp(logstd)) ** 2).sum(dim=1) + 0.5 * LOG_2PI * a.shape[1] + logstd.sum()


def tf_max(x, y):
    return torch.where(x >= y, x, y)


class Ref:
    """Parameters, Adam state and one `update` per minibatch, all float64."""

    def __init__(self, P, case):
        self.case = case
        self.pi, self.vf = tower_shapes(case)
        self.T = OrderedDict((n, torch.tensor(np.asarray(a, np.float64))) for n, a in P.items())
        self.trainable = [n for n in self.T if not n.startswith("model/q/")]
        self.m = {n: torch.zeros_like(self.T[n]) for n in self.trainable}
        self.v = {n: torch.zeros_like(self.T[n]) for n in self.trainable}
        self.t = 0

    def act(self, obs, eps=None):
        with torch.no_grad():
            mean, v = forward64(self.T, torch.tensor(np.asarray(obs, np.float64)), self.pi, self.vf)
            ls = self.T["model/pi/logstd:0"][0]
            a = mean if eps is None else mean + torch.exp(ls) * torch.tensor(np.asarray(eps, np.float64))
            return a.numpy(), v.numpy(), neglogp64(a, mean, ls).numpy()

    def update(self, mb, lr, apply=True):
        """mb: dict of float64 arrays obs, act, old_v, old_nlp, adv, ret.  Returns mean, v, the clipped gradients, the five
        diagnostics and the smallest distance of any row from a branch boundary."""
        c = self.case
        clip = c.get("cliprange", 0.2)
        cvf = c.get("cliprange_vf", None)
        cvf = clip if cvf is None else cvf
        ent_coef, vf_coef, mgn = c.get("ent_coef", 0.01), c.get("vf_coef", 0.5), c.get("max_grad_norm", 0.5)
        T = OrderedDict((n, p.clone().requires_grad_(n in self.trainable)) for n, p in self.T.items())
        t = {k: torch.tensor(np.asarray(a, np.float64)) for k, a in mb.items()}
        mean, v = forward64(T, t["obs"], self.pi, self.vf)
        ls = T["model/pi/logstd:0"][0]
        nlp = neglogp64(t["act"], mean, ls)
        adv = t["adv"]
        adv_n = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        ratio = torch.exp(t["old_nlp"] - nlp)
        rd = ratio.detach()
        l1, l2 = -adv_n * ratio, -adv_n * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
        pg = tf_max(l1, l2).mean()
        margin = min(float((rd - (1.0 - clip)).abs().min()), float((rd - (1.0 + clip)).abs().min()))
        e1 = (v - t["ret"]) ** 2
        if cvf >= 0:
            dlt = v - t["old_v"]
            vclip = t["old_v"] + torch.clamp(dlt, -cvf, cvf)
            e2 = (vclip - t["ret"]) ** 2
            vfl = 0.5 * tf_max(e1, e2).mean()
            margin = min(margin, float((dlt.detach().abs() - cvf).abs().min()))
            outside = dlt.detach().abs() > cvf       # (inside the clip the two errors are the same number: no branch to miss)
            if bool(outside.any()):
                margin = min(margin, float((e1 - e2).detach().abs()[outside].min()))
        else:
            vfl = 0.5 * e1.mean()
        entropy = (ls + 0.5 * (LOG_2PI + 1.0)).sum()
        loss = pg - ent_coef * entropy + vf_coef * vfl
        grads = torch.autograd.grad(loss, [T[n] for n in self.trainable])
        G = OrderedDict((n, g.detach()) for n, g in zip(self.trainable, grads))
        if mgn is not None and mgn > 0:
            norm = torch.sqrt(sum((g ** 2).sum() for g in G.values()))
            sc = mgn / max(float(norm), mgn)
            G = OrderedDict((n, g * sc) for n, g in G.items())
        diag = np.array([float(pg.detach()), float(vfl.detach()), float(entropy.detach()), float(0.5 * ((nlp.detach() - t["old_nlp"]) ** 2).mean()),
                         float(((rd - 1.0).abs() > clip).double().mean())])
        if apply:
            self.t += 1
            lr_t = lr * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t)
            for n in self.trainable:
                self.m[n] = self.m[n] + (G[n] - self.m[n]) * (1 - 0.9)
                self.v[n] = self.v[n] + (G[n] ** 2 - self.v[n]) * (1 - 0.999)
                self.T[n] = self.T[n] - lr_t * self.m[n] / (torch.sqrt(self.v[n]) + 1e-5)
        return dict(mean=mean.detach().numpy(), v=v.detach().numpy(), grads=OrderedDict((n, g.numpy()) for n, g in G.items()),
                    diag=diag, margin=margin, clipfrac_rows=int(((rd - 1.0).abs() > clip).sum()))


# ------------------------------------------------------------------------------------------------- seeded cases
def make_case(name, seed=None, noptepochs=2, lr=2.5e-4, **over):
    """seed None: the seed the table fixes for the case (0 where it names none)"""
    c = case_args(name)
    c.update(over)
    seed = c.get("seed", 0) if seed is None else seed
    c.update(name=name, seed=seed, noptepochs=noptepochs, lr=lr)
    pi, vf = tower_shapes(c)
    rng = np.random.default_rng(1000 + seed)
    n_envs, T, od, A = c["n_envs"], c["n_steps"], c["obs_dim"], c["A"]
    c["P"] = init_params(od, A, pi, vf, seed)
    ref = Ref(c["P"], c)
    obs = rng.normal(0.0, 1.0, (n_envs, T, od)).astype(np.float32)
    eps = rng.normal(0.0, 1.0, (n_envs, T, A)).astype(np.float32)
    a64, v64, nlp64 = ref.act(obs.reshape(-1, od), eps.reshape(-1, A))
    # the rollout as an OLDER policy left it: actions around the current means, old values and neglogps moved off the current ones
    # so that clipped and unclipped rows, on both sides, all occur
    c["obs"], c["eps"] = obs, eps
    c["act"] = a64.reshape(n_envs, T, A).astype(np.float32)
    c["old_v"] = (v64.reshape(n_envs, T) + rng.normal(0.0, 0.3, (n_envs, T))).astype(np.float32)
    c["old_nlp"] = (nlp64.reshape(n_envs, T) + rng.normal(0.0, 0.25, (n_envs, T))).astype(np.float32)
    c["rew"] = rng.normal(0.0, 1.0, (n_envs, T)).astype(np.float32)
    done = (rng.random((n_envs, T)) < 0.15).astype(np.float32)
    c["done"] = done
    c["last_obs"] = rng.normal(0.0, 1.0, (n_envs, od)).astype(np.float32)
    c["last_done"] = (rng.random(n_envs) < 0.3).astype(np.float32)
    R = n_envs * T
    prng = np.random.RandomState(seed)
    c["perm"] = np.stack([prng.permutation(R) for _ in range(noptepochs)]).astype(np.int32)
    return c


def engine_config(c):
    return _capi.make_ppo_config(c["obs_dim"], c["A"], n_envs=c["n_envs"], n_steps=c["n_steps"], nminibatches=c["nmb"],
                                 pi_layers=c["pi"], vf_layers=c["vf"], gamma=c.get("gamma", 0.99), lam=c.get("lam", 0.95), lr=c["lr"],
                                 ent_coef=c.get("ent_coef", 0.01), vf_coef=c.get("vf_coef", 0.5),
                                 max_grad_norm=c.get("max_grad_norm", 0.5), cliprange=c.get("cliprange", 0.2),
                                 cliprange_vf=c.get("cliprange_vf", None), seed=c["seed"])


def make_engine(c, backend=None, lib_path=None):
    cfg, ppo = engine_config(c)
    eng = PpoEngine(cfg, ppo, backend=backend, lib_path=lib_path)
    eng.set_parameters(c["P"])
    return eng


def place_and_finish(eng, c):
    """The case's rollout into the handle, last values + GAE on the engine; returns (adv, ret) [n_envs, n_steps] as it formed them."""
    eng.place_rollout(c["obs"], c["act"], c["old_v"], c["old_nlp"], c["rew"], c["done"])
    eng.finish(c["last_obs"], c["last_done"])
    shp = (c["n_envs"], c["n_steps"])
    return eng.fetch("ppo_adv", shp), eng.fetch("ppo_ret", shp)


def minibatches(c, adv, ret):
    """The minibatches of the case in update order, float64, rows as stable-baselines flattens them (env-major)."""
    R, od, A = c["n_envs"] * c["n_steps"], c["obs_dim"], c["A"]
    flat = dict(obs=c["obs"].reshape(R, od), act=c["act"].reshape(R, A), old_v=c["old_v"].reshape(R), old_nlp=c["old_nlp"].reshape(R),
                adv=np.asarray(adv).reshape(R), ret=np.asarray(ret).reshape(R))
    mb = R // c["nmb"]
    for e in range(c["noptepochs"]):
        for k in range(c["nmb"]):
            idx = c["perm"][e, k * mb:(k + 1) * mb]
            yield {n: np.asarray(a[idx], np.float64) for n, a in flat.items()}


def close_fwd(x, ref, what):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    d = np.abs(x - ref)
    assert x.shape == ref.shape, what
    assert (d <= 1e-5 + 1e-4 * np.abs(ref)).all(), "%s: max |d| %.3e" % (what, d.max())


def close_grads(G, ref, what=""):
    for n, g in ref.items():
        d = np.abs(np.asarray(G[n], np.float64) - g).max()
        assert d <= 1e-3 * max(np.abs(g).max(), 1e-30), "%s gradient %s: max |d| %.3e against max |g| %.3e" % (what, n, d, np.abs(g).max())


def close_params(P, ref, lr, n_updates):
    for n in ref.trainable:
        d = np.abs(np.asarray(P[n], np.float64) - ref.T[n].numpy())
        assert d.max() <= 0.3 * lr * n_updates + 1e-7, "param %s: max |d| %.3e (lr %.1e, %d updates)" % (n, d.max(), lr, n_updates)
        assert d.mean() <= 0.02 * lr * n_updates + 1e-9, "param %s: mean |d| %.3e" % (n, d.mean())


# ------------------------------------------------------------------------------------------------- the checks both builds run
def check_step_and_gae(eng, c):
    """model.step for n_steps steps with handed-over noise: actions / values / neglogps against the float64 policy, every slot of
    the rollout as written, the state errors of the protocol, then GAE bit for bit against the NumPy float32 restatement."""
    import pytest
    ref = Ref(c["P"], c)
    n, T, A, od = c["n_envs"], c["n_steps"], c["A"], c["obs_dim"]
    with pytest.raises(_capi.GrlError, match="no open slot"):
        eng.rewards(np.zeros(n))
    with pytest.raises(_capi.GrlError, match="not full"):
        eng.finish(c["last_obs"], c["last_done"])
    with pytest.raises(_capi.GrlError, match="no finished rollout"):
        eng.train(c["perm"])
    acts, vals, nlps = np.zeros((n, T, A), np.float32), np.zeros((n, T), np.float32), np.zeros((n, T), np.float32)
    for t in range(T):
        a, v, p = eng.step(c["obs"][:, t], c["done"][:, t], c["eps"][:, t])
        a64, v64, p64 = ref.act(c["obs"][:, t], c["eps"][:, t])
        close_fwd(a, a64, "action"); close_fwd(v, v64, "value"); close_fwd(p, p64, "neglogp")
        acts[:, t], vals[:, t], nlps[:, t] = a, v, p
        if t == 0:
            # (n_steps = 1: the only slot is open AND the rollout holds every step it can; grl_ppo_step names the latter first)
            with pytest.raises(_capi.GrlError, match="still open" if T > 1 else "rollout is full"):
                eng.step(c["obs"][:, t], c["done"][:, t], c["eps"][:, t])
        eng.rewards(c["rew"][:, t])
    with pytest.raises(_capi.GrlError, match="rollout is full"):
        eng.step(c["obs"][:, 0], c["done"][:, 0], c["eps"][:, 0])
    assert np.array_equal(eng.fetch("ppo_obs", (n, T, eng.ldo))[:, :, :od], c["obs"])
    assert not eng.fetch("ppo_obs", (n, T, eng.ldo))[:, :, od:].any()
    assert np.array_equal(eng.fetch("ppo_act", (n, T, A)), acts)
    assert np.array_equal(eng.fetch("ppo_old_v", (n, T)), vals) and np.array_equal(eng.fetch("ppo_old_nlp", (n, T)), nlps)
    assert np.array_equal(eng.fetch("ppo_rew", (n, T)), c["rew"]) and np.array_equal(eng.fetch("ppo_done", (n, T)), c["done"])
    eng.finish(c["last_obs"], c["last_done"])
    last_v = eng.fetch("ppo_last_v", (n,))
    close_fwd(last_v, ref.act(c["last_obs"])[1], "last values")
    adv, ret = gae_np(c["rew"], vals, c["done"], last_v, c["last_done"], 0.99, 0.95)
    assert np.array_equal(eng.fetch("ppo_adv", (n, T)).view(np.uint32), adv.view(np.uint32))
    assert np.array_equal(eng.fetch("ppo_ret", (n, T)).view(np.uint32), ret.view(np.uint32))
    eng.train(c["perm"])
    assert eng.metrics().shape == (c["noptepochs"] * c["nmb"], 5)
    eng.step(c["obs"][:, 0], c["done"][:, 0], c["eps"][:, 0])      # the rollout is empty again: slot 0
    assert np.array_equal(eng.fetch("ppo_obs", (n, T, eng.ldo))[:, 0, :od], c["obs"][:, 0])


def check_update(eng, c):
    """A placed rollout, GAE on the engine (bits of the NumPy restatement), then noptepochs * nminibatches updates: the five
    diagnostics of every update, mean / v and the clipped gradients of the last one, the parameters at the end."""
    adv, ret = place_and_finish(eng, c)
    last_v = eng.fetch("ppo_last_v", (c["n_envs"],))
    adv_np, ret_np = gae_np(c["rew"], c["old_v"], c["done"], last_v, c["last_done"], 0.99, 0.95)
    assert np.array_equal(adv.view(np.uint32), adv_np.view(np.uint32)) and np.array_equal(ret.view(np.uint32), ret_np.view(np.uint32))
    ref = Ref(c["P"], c)
    outs = [ref.update(mb, c["lr"]) for mb in minibatches(c, adv, ret)]
    B = c["n_envs"] * c["n_steps"] // c["nmb"]
    assert min(o["margin"] for o in outs) > MARGIN, "a row of the reference sits on a branch boundary: choose another seed"
    assert 0 < sum(o["clipfrac_rows"] for o in outs) < len(outs) * B      # clipped and unclipped rows both occur
    eng.train(c["perm"])
    m = eng.metrics()
    assert m.shape == (len(outs), 5)
    for u, o in enumerate(outs):
        print("update %d: engine %s reference %s margin %.3e" % (u, m[u], o["diag"], o["margin"]))
        assert np.allclose(m[u], o["diag"], rtol=1e-3, atol=1e-5), (u, m[u], o["diag"])
        assert round(float(m[u][4]) * B) == o["clipfrac_rows"]      # clipfrac counts rows: no row on the other side
    close_fwd(eng.fetch("ppo_mean", (B, c["A"])), outs[-1]["mean"], "mean of the last minibatch")
    close_fwd(eng.fetch("ppo_v", (B,)), outs[-1]["v"], "v of the last minibatch")
    close_grads(eng.get_gradients(), outs[-1]["grads"], "last update")
    close_params(eng.get_parameters(), ref, c["lr"], len(outs))
    P = eng.get_parameters()
    for n in ("model/q/w:0", "model/q/b:0"):
        assert np.array_equal(P[n], c["P"][n]), n


def check_act_routes_agree(c, make):
    """GRL_TUNE ppo_act=0 forces the launch list on a shape ppo_act_kernel takes: every step of the rollout gives the same
    actions, values and neglogps on both routes (the comparison test_launch_list_and_one_launch_act_agree makes at default_64_64).
    `make(c)` builds a handle; returns the plan dumps of the two handles when GRL_PLAN_DUMP is set."""
    import os
    outs = []
    for tune in (None, "ppo_act=0"):
        if tune:
            os.environ["GRL_TUNE"] = tune
        try:
            eng = make(c)
        finally:
            os.environ.pop("GRL_TUNE", None)
        steps = []
        for t in range(c["n_steps"]):
            steps.append(eng.step(c["obs"][:, t], c["done"][:, t], c["eps"][:, t]))
            eng.rewards(c["rew"][:, t])
        outs.append(steps)
        eng.close()
    for one, lst in zip(*outs):
        for a, b in zip(one, lst):
            assert np.allclose(a, b, rtol=1e-5, atol=1e-6), np.abs(a - b).max()


# ------------------------------------------------------------------------------------------------- device draws
DRAW_ENVS, DRAW_A, DRAW_CALLS = 257, 63, 16


def check_device_draws(make):
    """grl_act(deterministic=False, eps=NULL) draws its noise on the device (normal_pair_draw: Philox + Box-Muller, one pair per
    two action components, one counter per call).  257 rows x 63 components (odd: the last pair is half used) x 16 calls give
    N = 259 056 values z = (a - mean) / exp(logstd), held to what independent standard normals give: every bound is k = 6 standard
    errors of its statistic -- mean 1/sqrt(N), variance sqrt(2/N), excess kurtosis sqrt(24/N), a correlation coefficient over n pairs
    1/sqrt(n), which is at least 1/sqrt(N).  The output layer and logstd of the handle are zero, so a IS the draw, bit for bit, and
    ties are counted on the draws themselves: float32 normals do tie now and then (a NumPy float32 standard-normal array of the same
    size shows how often), the count is Poisson-like, and the bound is NumPy's count + 6 sqrt(count).  A pair reused across rows,
    calls or components gives thousands."""
    n, A, calls = DRAW_ENVS, DRAW_A, DRAW_CALLS
    c = dict(obs_dim=5, A=A, n_envs=n, n_steps=1, nmb=1, pi=(4,), vf=(4,), name="draws", seed=11, noptepochs=1, lr=2.5e-4)
    P = init_params(c["obs_dim"], A, c["pi"], c["vf"], c["seed"])
    for name in ("model/pi/w:0", "model/pi/b:0", "model/pi/logstd:0"):
        P[name] = np.zeros_like(P[name])
    c["P"] = P
    eng = make(c)
    obs = np.random.default_rng(5).normal(0.0, 1.0, (n, c["obs_dim"])).astype(np.float32)
    mean = eng.act(obs)
    assert not mean.any()
    a = np.stack([eng.act(obs, deterministic=False) for _ in range(calls)])
    eng.close()
    assert np.isfinite(a).all()
    z = (a.astype(np.float64) - mean) / np.exp(P["model/pi/logstd:0"][0].astype(np.float64))
    N = z.size
    assert N == 259056
    k = 6.0
    m, var = z.mean(), z.var()
    kurt = ((z - m) ** 4).mean() / var ** 2 - 3.0
    corr = lambda x, y: float(np.corrcoef(x.reshape(-1), y.reshape(-1))[0, 1])
    r_comp = corr(z[:, :, 0:A - 1:2], z[:, :, 1:A:2])      # the two halves of a pair
    r_rows = corr(z[:, :-1], z[:, 1:])
    r_call = corr(z[:-1], z[1:])
    ties = sum(row.size - np.unique(row).size for row in a.reshape(calls, -1))
    ties_np = sum(row.size - np.unique(row).size for row in np.random.default_rng(0).standard_normal((calls, n * A), dtype=np.float32))
    print("draws: mean %.3e var-1 %.3e kurtosis %.3e corr pair %.3e rows %.3e calls %.3e ties %d (NumPy %d)"
          % (m, var - 1.0, kurt, r_comp, r_rows, r_call, ties, ties_np))
    assert abs(m) <= k / np.sqrt(N)
    assert abs(var - 1.0) <= k * np.sqrt(2.0 / N)
    assert abs(kurt) <= k * np.sqrt(24.0 / N)
    for r in (r_comp, r_rows, r_call):
        assert abs(r) <= k / np.sqrt(N)
    assert ties <= ties_np + k * np.sqrt(max(ties_np, 1))
