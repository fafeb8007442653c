"""What a behaviour-cloning session (SAC handle) and a GAIL session (TRPO handle) compute on the g++ emulation build, bit for bit:
the plan lines, the launches as the profiler counts them, every result a caller can fetch, and the same again for a SECOND session
begun on the same handle after the first one ended (drop, graph teardown, fresh optimiser words).

tests/golden/session_parent.json was written by

    python tests/session_pin_util.py <emulation library> <out.json>

on the emulation build of the commit BEFORE the two sessions shared one record, one lifecycle and one Adam, with nothing else of
that change applied, and tests/test_hostemu_session_pin.py holds every later build to it with == on the parsed JSON.  The GPU
build plans other launches and rounds its GEMMs differently: emulation only.

Cases are existing ones of tests/bc_util.py (a -1 tail; widths that are no multiple of 16; an image extractor) and
tests/gail_util.py (odd sizes with a short expert batch; two blocks of the loss launch; the split first layer).

Per case {"plan": [...], "bytes": n (GAIL only), "first": {...}, "second": {...}}:
  plan    the `grl plan:` lines written between begin and end of the first session under GRL_PLAN_DUMP (the dry run of the size
          query, then the build)
  bytes   what grl_gail_query_sizes returned.  The behaviour-cloning size is not pinned; instead every session here, of either
          kind, runs in a buffer of exactly the queried size with guard words behind it, which must be untouched at the end
  BC      tags of one bc_train of three updates, tags of one bc_eval of the other two index rows, bc_losses() of both, the views
          bc_adam_m / bc_adam_v / bc_dmu, export_state() after bc_end
  GAIL    the rollout is placed (tu.place_and_finish's first half), the session begun as gu.check_updates does, the statistics set as
          gu.check_rewards does; tags of one gail_rewards, the rewritten rewards and gail_true_rew; then the rollout is finished
          (place_and_finish's second half: the reward pass wants a full rollout that is not closed yet, the update a closed one);
          tags of one gail_update of two updates, gail_losses(), the four blocks, gail_get_stats(), gail_logits, export_state()
          after gail_end
Arrays are recorded as the hex of their bytes up to 256 bytes and as "sha256:<digest of the bytes>" beyond (the moments of an image
policy are 5 MB of hex): equality of the record is equality of every bit either way."""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "deep-rl-grasping_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)

import bc_util as bu
import gail_util as gu
import parity_util as pu
import trpo_util as tu
from hostemu_backend import NumpyHostBackend

BC_CASES = ("mlp_b17_tail3", "narrow_24_40", "depth_augmented")
GAIL_CASES = ("odd_37", "two_blocks", "wide_obs")
CASES = ["bc " + n for n in BC_CASES] + ["gail " + n for n in GAIL_CASES]
GUARD = 64           # floats behind every allocation


class GuardedBackend(NumpyHostBackend):
    """Allocations of exactly the bytes asked for (rounded up to a float), a block of NaN-patterned guard words behind each."""
    PATTERN = 0x7fc5a5a5

    def __init__(self):
        self.blocks = []

    def alloc_f32(self, nbytes):
        n = (nbytes + 3) // 4
        full = np.zeros(n + GUARD, np.float32)
        full[n:].view(np.uint32)[:] = self.PATTERN
        self.blocks.append((nbytes, full))
        return full[:n]

    def assert_guards_untouched(self):
        for nbytes, full in self.blocks:
            assert (full[(nbytes + 3) // 4:].view(np.uint32) == self.PATTERN).all(), "a write beyond a buffer of %d bytes" % nbytes


def enc(a):
    b = np.ascontiguousarray(a).tobytes() if not isinstance(a, (bytes, bytearray)) else bytes(a)
    return b.hex() if len(b) <= 256 else "sha256:" + hashlib.sha256(b).hexdigest()


@contextlib.contextmanager
def plan_lines(out):
    """GRL_PLAN_DUMP for the block; the `grl plan:` lines the library wrote to file descriptor 2 meanwhile are appended to out."""
    sys.stderr.flush()
    saved, before = os.dup(2), os.environ.get("GRL_PLAN_DUMP")
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["GRL_PLAN_DUMP"] = "1"
        try:
            yield
        finally:
            if before is None:
                os.environ.pop("GRL_PLAN_DUMP", None)
            else:
                os.environ["GRL_PLAN_DUMP"] = before
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            text = f.read().decode()
            out.extend(l for l in text.splitlines() if l.startswith("grl plan:"))
            sys.stderr.write("".join(l + "\n" for l in text.splitlines() if not l.startswith("grl plan:")))


def profiled(eng, call):
    eng.profile(True)
    call()
    prof = eng.profile_dump()
    eng.profile(False)
    return {t: [v["launches"], int(v["flops"]), int(v["bytes"])] for t, v in sorted(prof.items())}


def bc_session(eng, c, plan):
    bb, A = c["bc_batch"], c["spec"].act_dim
    r = {}
    with plan_lines(plan):
        table = bu.begin(eng, c)
        r["train_tags"] = profiled(eng, lambda: eng.bc_train(table, c["bc_idx"]))
        r["train_losses"] = enc(eng.bc_losses())
        r["eval_tags"] = profiled(eng, lambda: eng.bc_eval(table, c["bc_idx"][1:3]))
        r["eval_losses"] = enc(eng.bc_losses())
        n = bu.n_trained(eng)
        r["bc_adam_m"], r["bc_adam_v"] = enc(eng.fetch("bc_adam_m", (n,))), enc(eng.fetch("bc_adam_v", (n,)))
        r["bc_dmu"] = enc(eng.fetch("bc_dmu", (bb, (A + 3) // 4 * 4)))
        eng.bc_end()
    r["state"] = enc(eng.export_state())
    return r


def gail_session(eng, c, plan):
    T, b = c["T"], c["batch"]
    r = {}
    eng.place_rollout(c["obs"][None], c["act"][None], c["vpred"][None], c["nlp"][None], c["rew"][None], c["es"][None])
    with plan_lines(plan):
        table = gu.begin(eng, c)
        d = gu.Disc(c)
        d.rms_update(c["exp_obs"])
        eng.gail_set_stats(d.sum, d.sumsq, d.count)
        r["rewards_tags"] = profiled(eng, eng.gail_rewards)
        r["ppo_rew"] = enc(eng.fetch("ppo_rew", (T,)))
        r["gail_true_rew"] = enc(eng.fetch("gail_true_rew", (T,)))
        eng.finish(c["last_obs"], [c["last_es"]])
        r["update_tags"] = profiled(eng, lambda: eng.gail_update(table, c["gen_idx"][:2], c["exp_idx"][:2]))
        r["losses"] = enc(eng.gail_losses())
        for blk in ("gail_params", "gail_adam_m", "gail_adam_v", "gail_grads"):
            r[blk] = {name: enc(a) for name, a in eng.gail_get_parameters(blk).items()}
        s, q, n = eng.gail_get_stats()
        r["stats"] = [enc(s), enc(q), enc(np.float64(n))]
        r["gail_logits"] = enc(eng.fetch("gail_logits", (2 * b,)))
        eng.gail_end()
    r["state"] = enc(eng.export_state())
    return r


def capture(name, lib):
    kind, case = name.split(" ")
    be = GuardedBackend()
    if kind == "bc":
        c = bu.make_case(case)
        eng, session = pu.engine_setup(c, backend=be, lib_path=lib), bc_session
    else:
        c = gu.make_case(case)
        eng, session = tu.make_engine(c, backend=be, lib_path=lib), gail_session
    try:
        n_handle = len(be.blocks)
        out, plan = {}, []
        out["first"] = session(eng, c, plan)
        out["plan"] = plan
        out["second"] = session(eng, c, [])
        assert len(be.blocks) == n_handle + 2, "a session allocates ONE buffer, of the queried size"
        if kind == "gail":
            assert be.blocks[n_handle][0] == be.blocks[n_handle + 1][0]
            out["bytes"] = be.blocks[n_handle][0]
        be.assert_guards_untouched()
        return out
    finally:
        eng.close()


if __name__ == "__main__":
    lib, out = sys.argv[1], sys.argv[2]
    os.environ.pop("GRL_TUNE", None)
    with open(out, "w") as f:
        json.dump({name: capture(name, lib) for name in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
