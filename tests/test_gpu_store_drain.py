"""GRL_TUNE store_drain=<mask> (csrc/store_drain.h; README.md, "Switches"): tensor groups of the SAC CNN plan whose 16-byte
stores leave the L2 write-through instead of waiting for the kernel boundary.  Only the cache policy of stores moves: every case
runs all groups (127) against none (0) and asks for the same bits in every parameter and every gradient.

Shapes: B = 16 is the smallest batch at which the riding image gather and the fused heads are planned; B = 32 gives more than one
row block per chain type and more than one slab split; the byte-colour RGB-D ring runs grouped rider rows and the 4-channel
stack.  Three explicit minibatches, then device-RNG calls of 5 and 2 updates: first / middle / last launch lists and both image
buffers."""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu


def run(monkeypatch, case, tune, oracle_first=None):
    monkeypatch.setenv("GRL_TUNE", tune)
    eng = pu.engine_setup(case)
    try:
        eng.train(1, case["idx"][:1], case["eps"][:1])
        if oracle_first is not None:
            pu.compare_first_step(eng, case, oracle_first)
        for s in (1, 2):
            eng.train(1, case["idx"][s:s + 1], case["eps"][s:s + 1])
        g_explicit = eng.get_gradients()
        eng.train_device(5)
        eng.train_device(2)
        return eng.get_parameters(), g_explicit, eng.get_gradients()
    finally:
        eng.close()
        monkeypatch.delenv("GRL_TUNE")


def same_bits(ref, got):
    for a, b in zip(ref, got):
        assert list(a) == list(b)
        for n in a:
            assert np.array_equal(a[n], b[n]), n


@pytest.mark.parametrize("kw", [dict(kind="depth", B=16), dict(kind="depth", B=32), dict(kind="rgbd", rgb_u8=True, B=16)],
                         ids=["depth_b16", "depth_b32", "rgbd_u8_b16"])
def test_all_groups_write_through_leave_the_same_bits(monkeypatch, kw):
    case = pu.make_case(extractor="augmented", n_replay=64, n_steps=3, **kw)
    same_bits(run(monkeypatch, case, "store_drain=0"), run(monkeypatch, case, "store_drain=127"))


def test_per_layer_route_write_through_matches_the_oracle_and_the_plain_stores(monkeypatch):
    """GRL_TUNE conv_stack=0: the convolution outputs (a1, a2, a3) go through igemm2's wide epilogue, where the per-problem flag
    VF_C_DRAIN selects the policy.  The first update against the oracle at the default plan's tolerances
    (parity_util.compare_first_step), and everything against the same route with plain stores."""
    case = pu.make_case(extractor="augmented", kind="depth", B=16, n_replay=64, n_steps=3)
    ref, _ = pu.oracle_run(case)
    same_bits(run(monkeypatch, case, "conv_stack=0,store_drain=0"),
              run(monkeypatch, case, "conv_stack=0,store_drain=127", oracle_first=ref[0]))
