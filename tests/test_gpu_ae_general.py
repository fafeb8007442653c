"""Auto-encoder of any supported configuration on the GPU (libgrl.so, general launch plan of csrc/plan_ae.inl): the cases of
ae_general_util.CASES against the float32 restatement, the shipped network down the general route against the restatement and
against the tuned route, and run-to-run equality of the bits (the new kernels use no atomics)."""
import numpy as np
import pytest

import ae_general_util as gu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(gu.CASES))
def test_general_route_matches_the_restatement(name):
    gu.ae_general_check(name)


def test_shipped_network_general_route_against_restatement_and_tuned_route(monkeypatch):
    gu.shipped_general_check(monkeypatch)


def test_two_runs_give_equal_bits():
    ks, fs, dim, alpha, B = gu.CASES["dim7_b5"]
    a = gu.run_engine((ks, fs, dim, alpha), B)
    b = gu.run_engine((ks, fs, dim, alpha), B)
    assert a["loss"] == b["loss"]
    for k in ("enc", "rec"):
        assert np.array_equal(a[k], b[k])
    for s in range(3):
        assert np.array_equal(a["out"][s], b["out"][s])
    for n in a["params"]:
        assert np.array_equal(a["params"][n], b["params"][n]) and np.array_equal(a["grads"][n], b["grads"][n])
