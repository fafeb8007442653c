"""The launches of one training call per plan, as the profiler counts them: tag -> [launches, FLOPs per launch, bytes per launch]
(grl_profile_enable(1), the call, grl_profile_dump), and the handle's exported host state as hex.  The plan dumps pin the GEMM
launches and the SAC / Q op lists; this pins the op lists nothing else names tag by tag -- PPO2, TRPO, the auto-encoder's two
routes, behaviour cloning -- together with one case of each other plan that shares their launch constructors (the slab
reduction, Adam, the stack weight gradients, the tiled clip + Adam: csrc/engine.hip).

tests/golden/launch_tags_parent.json was written by

    python tests/launch_tags_util.py <emulation library> <out.json>

on the emulation build of the commit BEFORE those constructors were shared, and tests/test_hostemu_launch_tags.py holds every
later build to it.  The GPU build plans other launches (matrix-core chains, 16-byte reductions): emulation only.

Cases, the smallest that reach every branch of the shared code: unequal tower depths (the tower mask at the deepest level), a split
first layer, a PPO2 handle without gradient clipping (plain Adam), TRPO without and with a value minibatch (T < 128 has none),
the shipped auto-encoder and the smallest general one at batch 8, behaviour cloning on vectors and on images, DQN with the
per-variable clip and BDQ on the wide route (full update and the split compute / apply pair each), the smallest SAC MLP."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "deep-rl-grasping_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)

import ae_general_util as au
import bc_util as bu
import parity_util as pu
import ppo_norm_util as nu
import ppo_util as ppu
import q_parity_util as qu
import trpo_util as tu
from grasp_rl.autoencoder import AeEngine, SHIPPED_NET
from hostemu_backend import NumpyHostBackend

AE_B = 8
SAC_MLP = dict(extractor="mlp", B=8, n_replay=32, normalize="reward")      # tests/test_hostemu_plan.py: mlp_norm_reward_only


def _ppo(name):
    def run(lib):
        c = ppu.make_case(name)
        eng = ppu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)
        ppu.place_and_finish(eng, c)
        return eng, lambda: eng.train(c["perm"])
    return run


def _trpo(name, **over):
    def run(lib):
        c = tu.make_case(name, **over)
        eng = tu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)
        tu.place_and_finish(eng, c)
        return eng, lambda: eng.update(c["vf_perm"])
    return run


def _ae(net):
    def run(lib):
        P0, x = au.case_inputs(net, AE_B, n_steps=1)
        eng = AeEngine(AE_B, 2e-4, act_batch=4, backend=NumpyHostBackend(), lib_path=lib, net=net)
        eng.set_parameters(P0)
        return eng, lambda: eng.train_batches(x)
    return run


def _bc(name):
    def run(lib):
        c = bu.make_case(name)
        eng = pu.engine_setup(c, backend=NumpyHostBackend(), lib_path=lib)
        table = bu.begin(eng, c)
        return eng, lambda: eng.bc_train(table, c["bc_idx"][:1])
    return run


def _q(name, **over):
    def run(lib):
        c = qu.make_q_case(**qu.case_args(name, **over))
        assert c["cfg"].q_grad_clip > 0 and c["cfg"].q_layer_norm == 0
        eng = qu.q_engine_setup(c, backend=NumpyHostBackend(), lib_path=lib)

        def call():      # a full update, then the split pair (the launches of their own: reduce_slabs | clip | adam)
            eng.train(1, c["idx"][:1], c["weights"][:1])
            eng.compute_grads(c["idx"][1:2], c["weights"][1:2])
            eng.apply_grads(1.0)
        return eng, call
    return run


def _sac(lib):
    c = pu.make_case(n_steps=1, **SAC_MLP)
    eng = pu.engine_setup(c, backend=NumpyHostBackend(), lib_path=lib)
    return eng, lambda: eng.train(1, c["idx"][:1], c["eps"][:1])


_PPO_PARENT = {"ppo": _ppo, "trpo": _trpo}
CASES = dict([("%s %s" % (kind, name), _PPO_PARENT[kind](name)) for kind, name in nu.PARENT_CASES] + [
    ("ppo no_vf_clip", _ppo("no_vf_clip")),                      # max_grad_norm None -> 0: adam alone
    ("trpo odd T128", _trpo("odd", T=128)),                      # ... with one value minibatch
    ("ae shipped", _ae(SHIPPED_NET)),
    ("ae k3_f8_16_32", _ae(au.CASES["k3_f8_16_32"][:4])),
    ("bc narrow_24_40", _bc("narrow_24_40")),
    ("bc depth_nature", _bc("depth_nature")),
    ("q dqn", _q("dqn")),                                        # narrow, per-variable clip
    ("q bdq obs8200", _q("bdq", obs_dim=8200)),                  # 8200 x 16 floats: the wide route
    ("sac mlp", _sac),
])


def capture(name, lib):
    """{"tags": {tag: [launches, FLOPs per launch, bytes per launch]}, "state": hex} of case `name` on library `lib`."""
    eng, call = CASES[name](lib)
    try:
        eng.profile(True)
        call()
        prof = eng.profile_dump()
        eng.profile(False)
        tags = {t: [v["launches"], int(v["flops"]), int(v["bytes"])] for t, v in sorted(prof.items())}
        return {"tags": tags, "state": eng.export_state().hex()}
    finally:
        eng.close()


if __name__ == "__main__":
    lib, out = sys.argv[1], sys.argv[2]
    os.environ.pop("GRL_TUNE", None)
    with open(out, "w") as f:
        json.dump({name: capture(name, lib) for name in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
