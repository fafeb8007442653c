"""``DQN.learn`` / ``BDQ.learn`` with the VecNormalize statistics on the MI355X (``device_norm=True``) against the host path
(tests/q_device_norm_learn_util.py): parameters, replay arrays, the pickled statistics, counters and the exploration generator
bit for bit, no statistics push and no five-copy append after the first step, and a checkpoint that continues."""
import pytest

import q_device_norm_learn_util as ql

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("algo,per,n", ql.CASES)
def test_learn_with_device_statistics_equals_host_statistics(algo, per, n, monkeypatch):
    monkeypatch.delenv("GRL_DEVICE_NORM", raising=False)
    ql.check_device_equals_host(algo, per, n)


def test_checkpoint_saved_with_device_statistics_continues(tmp_path, monkeypatch):
    ql.check_checkpoint_continues("bdq", True, tmp_path, monkeypatch)
