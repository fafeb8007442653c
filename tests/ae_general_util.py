"""Auto-encoder of any supported configuration: a float32 torch restatement of oracle/autoencoder.py:AeOracle parametrised in
the bottleneck channels f2 and the LeakyReLU slope (the oracle fixes 32 and 0.1), the cases of the general launch plan and the
engine-vs-restatement check that the CPU (emulation build) and GPU tests share.  The restatement uses the oracle's own
operations (`_conv_same`, `leaky_relu`, `repeat_interleave`, the Keras-Adam lines) and is held against `AeOracle` bit for bit
by tests/test_hostemu_ae_general.py before anything else relies on it."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from grasp_rl.autoencoder import AeEngine, PARAM_NAMES, SHIPPED_NET, param_shapes
from oracle import autoencoder as oae

# name -> (kernel sizes, filters, encoding_dim, alpha, batch)
CASES = {
    "dim7_b5": ((7, 5, 3), (32, 32, 32), 7, 0.1, 5),
    "k3_f8_16_32": ((3, 3, 3), (8, 16, 32), 100, 0.1, 4),
    "k9_4_1": ((9, 4, 1), (32, 32, 32), 33, 0.1, 4),
    "f64_12_16": ((5, 5, 5), (64, 12, 16), 128, 0.1, 4),
    "f4_dim1024": ((3, 3, 3), (4, 4, 4), 1024, 0.1, 4),
    "alpha0": ((7, 5, 3), (32, 32, 32), 100, 0.0, 4),
    "alpha03": ((7, 5, 3), (32, 32, 32), 100, 0.3, 4),
}
SHIPPED_GENERAL_B = 8        # `shipped_general`: the shipped network under GRL_TUNE=ae_general=1

# Tolerances of tests/ae_parity_util.py:ae_check
OUT_ATOL, OUT_RTOL, LOSS_RTOL, GRAD_REL, PARAM_MAX, PARAM_MEAN, ENC_ATOL, ENC_RTOL = 2e-5, 1e-4, 1e-4, 1e-3, 0.3, 0.02, 2e-5, 2e-4
# A case whose reductions are longer than the shipped network's may add to them four times the deviation of this float32
# restatement from the same restatement in float64 on the same inputs and parameters (the rule of the wide Q
# cases).  Measured on the CPU by `float64_deviation(case)`; per case {quantity: deviation}.  `k9_4_1` is the one case with
# a longer reduction (81 * 32 products per output of conv2d_6, against 49 * 32): out 2.52e-07, loss 8.02e-08 relative,
# gradients 2.96e-07 of max |g|, encodings 6.52e-08 -- the allowance moves ae_check's bounds by about 5 % (out) or less.
F64_DEVIATION = {
    "k9_4_1": {"out": 2.52e-7, "loss_rel": 8.02e-8, "grad_rel": 2.96e-7, "enc": 6.52e-8},
}


def init_params(net, seed=0):
    """Keras defaults as oracle.autoencoder.init_params draws them, for the shapes of `net`."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shp in zip(PARAM_NAMES, param_shapes(net)):
        if name.endswith("bias"):
            P[name] = np.zeros(shp, np.float32)
        else:
            rf = int(np.prod(shp[:-2])) if len(shp) == 4 else 1
            lim = np.sqrt(6.0 / (shp[-2] * rf + shp[-1] * rf))
            P[name] = rng.uniform(-lim, lim, shp).astype(np.float32)
    return P


def _conv_same64(x_nhwc, w_hwio, b, stride):
    """oae._conv_same with the permuted kernel made contiguous: torch's float64 CPU convolution needs that for its weight
    gradient.  Used by the float64 yardstick only; the float32 reference calls the oracle's own function."""
    lo, hi = oae.tf_same_pad(x_nhwc.shape[1], w_hwio.shape[0], stride)
    x = F.pad(x_nhwc.permute(0, 3, 1, 2), (lo, hi, lo, hi))
    y = F.conv2d(x, w_hwio.permute(3, 2, 0, 1).contiguous(), stride=stride)
    return y.permute(0, 2, 3, 1) + b.reshape(1, 1, 1, -1)


class AeRestated:
    """AeOracle with the bottleneck channels taken from the parameters and the slope as an argument; dtype float32 (the
    reference of the tests) or float64 (the yardstick of its own rounding)."""

    def __init__(self, params, alpha=0.1, lr=2e-4, eps=1e-7, dtype=torch.float32):
        self.dtype = dtype
        self.P = {k: torch.tensor(np.asarray(v, np.float32), dtype=dtype, requires_grad=True) for k, v in params.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.P.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.P.items()}
        self.alpha, self.lr, self.eps, self.t = alpha, lr, eps, 0
        self.f2 = int(self.P["encoder/conv2d_3/kernel"].shape[3])
        self.conv = oae._conv_same if dtype == torch.float32 else _conv_same64

    def encode_t(self, x):
        P, h = self.P, x
        for i in (1, 2, 3):
            h = F.leaky_relu(self.conv(h, P["encoder/conv2d_%d/kernel" % i], P["encoder/conv2d_%d/bias" % i], oae.STRIDE), self.alpha)
        return F.leaky_relu(h.reshape(h.shape[0], -1) @ P["encoder/dense_1/kernel"] + P["encoder/dense_1/bias"], self.alpha)

    def forward(self, x):
        P = self.P
        z = self.encode_t(x)
        h = F.leaky_relu(z @ P["decoder/dense_2/kernel"] + P["decoder/dense_2/bias"], self.alpha).reshape(-1, 8, 8, self.f2)
        for i in (4, 5):
            h = h.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            h = F.leaky_relu(self.conv(h, P["decoder/conv2d_%d/kernel" % i], P["decoder/conv2d_%d/bias" % i], 1), self.alpha)
        h = h.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        return self.conv(h, P["decoder/conv2d_6/kernel"], P["decoder/conv2d_6/bias"], 1), z

    def step(self, x_np):
        x = torch.from_numpy(np.asarray(x_np, np.float32)).to(self.dtype)
        out, z = self.forward(x)
        loss = torch.mean((out - x) ** 2)
        grads = torch.autograd.grad(loss, list(self.P.values()))
        res = {"loss": float(loss.detach()), "out": out.detach().numpy().copy(), "z": z.detach().numpy().copy(),
               "grads": {k: g.numpy().copy() for k, g in zip(self.P, grads)}}
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t)
        lr_t = np.float32(lr_t) if self.dtype == torch.float32 else lr_t
        with torch.no_grad():
            for (k, p), g in zip(self.P.items(), grads):
                self.m[k].mul_(0.9).add_(g, alpha=0.1)
                self.v[k].mul_(0.999).addcmul_(g, g, value=0.001)
                p.sub_(lr_t * self.m[k] / (torch.sqrt(self.v[k]) + self.eps))
        return res

    def params(self):
        return {k: v.detach().numpy().copy() for k, v in self.P.items()}

    def encode(self, x_np):
        with torch.no_grad():
            return self.encode_t(torch.from_numpy(np.asarray(x_np, np.float32)).to(self.dtype)).numpy()

    def reconstruct(self, x_np):
        with torch.no_grad():
            return self.forward(torch.from_numpy(np.asarray(x_np, np.float32)).to(self.dtype))[0].numpy()


def case_inputs(net, B, n_steps=3, seed=0):
    """Parameters (non-zero biases) and the depth-like images of ae_check."""
    rng = np.random.default_rng(seed + 5)
    P0 = init_params(net, seed)
    for k in P0:
        if k.endswith("bias"):
            P0[k] = rng.normal(0, 0.05, P0[k].shape).astype(np.float32)
    x = np.zeros((n_steps * B, 64, 64, 1), np.float32)
    for i in range(x.shape[0]):
        r0, c0 = rng.integers(5, 40, 2)
        x[i, r0:r0 + 20, c0:c0 + 18, 0] = rng.uniform(0.2, 0.5, (20, 18))
    return P0, x


@functools.lru_cache(maxsize=None)
def reference_run(net, B, n_steps=3, lr=2e-4):
    """The restatement's three steps, computed once per (network, batch) and shared: per-step results, final parameters,
    encodings of 3 images.  Callers do not modify what they get."""
    P0, x = case_inputs(net, B, n_steps)
    ref = AeRestated(P0, alpha=net[3], lr=lr)
    steps = [ref.step(x[s * B:(s + 1) * B]) for s in range(n_steps)]
    return {"P0": P0, "x": x, "steps": steps, "params": ref.params(), "enc": ref.encode(x[:3])}


def float64_deviation(name, n_steps=3, lr=2e-4):
    """How far the float32 restatement is from itself in float64 (same inputs, same parameters at every step's start is not
    forced: both run their own three steps): max |d out|, relative loss, gradient deviation relative to max |g|, max |d enc|."""
    ks, fs, dim, alpha, B = CASES[name]
    net = (ks, fs, dim, alpha)
    P0, x = case_inputs(net, B, n_steps)
    a, b = AeRestated(P0, alpha, lr), AeRestated(P0, alpha, lr, dtype=torch.float64)
    dev = {"out": 0.0, "loss_rel": 0.0, "grad_rel": 0.0}
    for s in range(n_steps):
        ra, rb = a.step(x[s * B:(s + 1) * B]), b.step(x[s * B:(s + 1) * B])
        dev["out"] = max(dev["out"], float(np.abs(ra["out"] - rb["out"]).max()))
        dev["loss_rel"] = max(dev["loss_rel"], abs(ra["loss"] - rb["loss"]) / abs(rb["loss"]))
        if s == 0:
            for k in ra["grads"]:
                dev["grad_rel"] = max(dev["grad_rel"], float(np.abs(ra["grads"][k] - rb["grads"][k]).max() / np.abs(rb["grads"][k]).max()))
    dev["enc"] = float(np.abs(a.encode(x[:3]) - b.encode(x[:3])).max())
    return dev


def run_engine(net, B, backend=None, lib_path=None, n_steps=3, lr=2e-4, with_forward_only=True):
    """The sequence of ae_check on an engine of `net`: what it computed, as arrays."""
    P0, x = case_inputs(net, B, n_steps)
    eng = AeEngine(B, lr, act_batch=4, backend=backend, lib_path=lib_path, net=net)
    try:
        assert [n for n, *_ in eng.table] == PARAM_NAMES
        assert [tuple(r[3]) for r in eng.table] == param_shapes(net)
        eng.set_parameters(P0)
        got = {"loss": [], "out": [], "grads": None}
        for s in range(n_steps):
            got["loss"].append(eng.train_batches(x[s * B:(s + 1) * B]))
            got["out"].append(eng.reconstruction().copy())
            if s == 0:
                got["grads"] = {k: v.copy() for k, v in eng.get_gradients().items()}
        got["params"] = eng.get_parameters()
        if with_forward_only:
            got["enc"] = eng.encode(x[:3])
            got["rec"] = eng.reconstruct(x[:B + 1])
            got["params_after"] = eng.get_parameters()
        return got
    finally:
        eng.close()


def compare(got, want, n_steps=3, lr=2e-4, scale=1.0, extra=None):
    """`got` (run_engine) against `want` ({"steps", "params", "enc"}), bounds = scale * ae_check's (+ 4 * `extra` deviations).
    Prints every figure before it asserts."""
    ex = {k: 4.0 * v for k, v in (extra or {}).items()}
    for s in range(n_steps):
        ref = want["steps"][s]
        d = np.abs(got["out"][s] - ref["out"])
        bound = scale * (OUT_ATOL + OUT_RTOL * np.abs(ref["out"])) + ex.get("out", 0.0)
        print("step %d: max |d out| %.3e  loss %.8g vs %.8g" % (s, d.max(), got["loss"][s], ref["loss"]))
        assert (d <= bound).all(), "step %d: out off by %.3e" % (s, d.max())
        assert abs(got["loss"][s] - ref["loss"]) <= (scale * LOSS_RTOL + ex.get("loss_rel", 0.0)) * abs(ref["loss"]) + 1e-7, (got["loss"][s], ref["loss"])
    for n, g in want["steps"][0]["grads"].items():
        d, gm = np.abs(got["grads"][n] - g).max(), max(np.abs(g).max(), 1e-12)
        print("grad %s: max |d| %.3e of max |g| %.3e" % (n, d, gm))
        assert d <= (scale * GRAD_REL + ex.get("grad_rel", 0.0)) * gm + 1e-9, "grad %s: %.3e vs max %.3e" % (n, d, gm)
    for n in PARAM_NAMES:
        d = np.abs(got["params"][n] - want["params"][n])
        assert d.max() <= scale * PARAM_MAX * lr * n_steps + 1e-7, "param %s: max |d| %.3e" % (n, d.max())
        assert d.mean() <= scale * PARAM_MEAN * lr * n_steps + 1e-9, "param %s: mean |d| %.3e" % (n, d.mean())
    if "enc" in want and "enc" in got:
        d = np.abs(got["enc"] - want["enc"])
        print("encodings: max |d| %.3e" % d.max())
        assert got["enc"].shape == want["enc"].shape
        assert (d <= scale * (ENC_ATOL + ENC_RTOL * np.abs(want["enc"])) + ex.get("enc", 0.0)).all(), d.max()


def ae_general_check(name, backend=None, lib_path=None):
    """One case of CASES against the restatement: ae_check's sequence and bounds."""
    ks, fs, dim, alpha, B = CASES[name]
    net = (ks, fs, dim, alpha)
    want = reference_run(net, B)
    got = run_engine(net, B, backend=backend, lib_path=lib_path)
    compare(got, want, extra=F64_DEVIATION.get(name))
    # the encodings above belong to the restatement's final parameters; the forward-only pass is held against the restatement
    # at the ENGINE's parameters, for a batch that is no multiple of the engine's, and must leave the parameters alone
    rec_want = AeRestated(got["params"], alpha=alpha).reconstruct(want["x"][:B + 1])
    d = np.abs(got["rec"] - rec_want)
    print("reconstruct: max |d| %.3e" % d.max())
    assert got["rec"].shape == (B + 1, 64, 64, 1)
    assert (d <= OUT_ATOL + OUT_RTOL * np.abs(rec_want) + 4.0 * F64_DEVIATION.get(name, {}).get("out", 0.0)).all(), d.max()
    assert all(np.array_equal(got["params_after"][n], got["params"][n]) for n in PARAM_NAMES)
    return got


def shipped_general_check(monkeypatch, backend=None, lib_path=None):
    """The shipped network down the general route (GRL_TUNE=ae_general=1): against the restatement at ae_check's bounds, and
    against the tuned route on the same inputs at twice those bounds."""
    B = SHIPPED_GENERAL_B
    monkeypatch.delenv("GRL_TUNE", raising=False)
    tuned = run_engine(SHIPPED_NET, B, backend=backend, lib_path=lib_path)
    monkeypatch.setenv("GRL_TUNE", "ae_general=1")
    general = run_engine(SHIPPED_NET, B, backend=backend, lib_path=lib_path)
    monkeypatch.delenv("GRL_TUNE", raising=False)
    compare(general, reference_run(SHIPPED_NET, B))
    as_ref = {"steps": [{"out": tuned["out"][s], "loss": tuned["loss"][s], "grads": tuned["grads"]} for s in range(3)],
              "params": tuned["params"], "enc": tuned["enc"]}
    compare(general, as_ref, scale=2.0)
    d = np.abs(general["rec"] - tuned["rec"])
    assert (d <= 2.0 * (OUT_ATOL + OUT_RTOL * np.abs(tuned["rec"]))).all(), d.max()
    return tuned, general


def plan_text_and_table(lib_path, backend, capfd, B=8, act_batch=4, net=None):
    """What a handle prints under GRL_PLAN_DUMP (the caller has set it) plus its variable table, as one text."""
    capfd.readouterr()
    eng = AeEngine(B, 2e-4, act_batch=act_batch, backend=backend, lib_path=lib_path, net=net)
    text = capfd.readouterr().err
    for row in eng.table:
        text += "var %s %d %d %s %d\n" % (row[0], row[1], row[2], "x".join(map(str, row[3])), int(row[4]))
    eng.close()
    return text
