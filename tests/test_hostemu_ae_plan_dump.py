"""The shipped auto-encoder's launch plan is the parent's, byte for byte: tests/golden/ae_plan_dump_parent.txt holds what a
handle (batch 8, act_batch 4) of the emulation build printed under GRL_PLAN_DUMP -- size query and create -- and its variable
table, recorded before the general route (plan_ae_general) existed."""
import os

import ae_general_util as gu
from hostemu_backend import NumpyHostBackend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ae_plan_dump_parent.txt")


def test_shipped_plan_dump_and_variable_table_equal_the_parents(hostemu_lib, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    monkeypatch.delenv("GRL_TUNE", raising=False)
    text = gu.plan_text_and_table(hostemu_lib, NumpyHostBackend(), capfd)
    with open(GOLDEN) as f:
        assert text == f.read()
