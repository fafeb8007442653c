"""GRL_TUNE store_drain=<mask> on the emulation build (csrc/store_drain.h has a plain body there; the `hostemu_lib` fixture
compiles it): what GRL_PLAN_DUMP says about the mask in effect, that bits outside the seven groups are ignored, and that the host
logic the mask touches -- problem flags, kernel arguments, launch lists -- leaves the parameters alone."""
import os
import re

import numpy as np
import pytest

import parity_util as pu
from hostemu_backend import NumpyHostBackend

CNN = dict(extractor="augmented", kind="depth", B=16, n_replay=48)


def masks_in_dump(monkeypatch, capfd, hostemu_lib, tune, **kw):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    if tune is not None:
        monkeypatch.setenv("GRL_TUNE", tune)
    capfd.readouterr()
    case = pu.make_case(n_steps=1, **kw)
    pu.SacEngine(case["cfg"], backend=NumpyHostBackend(), lib_path=hostemu_lib).close()
    dump = capfd.readouterr().err
    return [int(m) for m in re.findall(r"^grl plan: store_drain +mask (\d+) ", dump, re.M)], dump


@pytest.mark.parametrize("tune,want", [("store_drain=0", 0), ("store_drain=5", 5), ("store_drain=127", 31),
                                       ("store_drain=1023", 31), ("store_drain=96", 0), ("conv_stack=0,store_drain=66", 2)])
def test_plan_dump_reports_the_mask_in_effect(hostemu_lib, monkeypatch, capfd, tune, want):
    """One line per planning run (the dry run of grl_query_sizes and grl_create).  Bits that name no built group are dropped:
    32 / 64 (Adam moments, parameters + targets: no gain) and everything above."""
    masks, dump = masks_in_dump(monkeypatch, capfd, hostemu_lib, tune, **CNN)
    assert len(masks) >= 1 and all(m == want for m in masks), dump
    assert "unknown key" not in dump, dump


def readme_default():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    row = re.search(r"^\| `store_drain` \| (\d+) \|", open(os.path.join(root, "README.md")).read(), re.M)
    return int(row.group(1))


def test_default_mask_is_the_one_the_readme_states(hostemu_lib, monkeypatch, capfd):
    monkeypatch.delenv("GRL_TUNE", raising=False)
    masks, dump = masks_in_dump(monkeypatch, capfd, hostemu_lib, None, **CNN)
    assert len(masks) >= 1 and all(m == readme_default() for m in masks), dump


def test_feature_vector_plans_have_no_mask(hostemu_lib, monkeypatch, capfd):
    """SAC CNN plans only: the MLP plan neither reads nor reports it (the key itself is still a row of the table)."""
    masks, dump = masks_in_dump(monkeypatch, capfd, hostemu_lib, "store_drain=127", extractor="mlp", B=16, n_replay=64)
    assert masks == [] and "unknown key" not in dump, dump


@pytest.mark.parametrize("route", ["", "conv_stack=0,"])
def test_emulated_parameters_do_not_depend_on_the_mask(hostemu_lib, monkeypatch, route):
    case = pu.make_case(n_steps=2, **CNN)

    def run(mask):
        monkeypatch.setenv("GRL_TUNE", "%sstore_drain=%d" % (route, mask))
        eng = pu.engine_setup(case, backend=NumpyHostBackend(), lib_path=hostemu_lib)
        for s in range(2):
            eng.train(1, case["idx"][s:s + 1], case["eps"][s:s + 1])
        eng.train(3)          # first / middle / last launch lists, both image buffers
        out = (eng.get_parameters(), eng.get_gradients())
        eng.close()
        return out
    ref, got = run(0), run(127)
    for a, b in zip(ref, got):
        assert all(np.array_equal(a[n], b[n]) for n in a)
