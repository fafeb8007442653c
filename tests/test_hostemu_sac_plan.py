"""The SAC launch plan against the record of the commit before csrc/plan_sac.inl became a list of steps (CPU, emulation build)."""
import os

import sac_plan_util as su

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_plans_connects_tables_and_arena_sizes_are_the_parent_commits(hostemu_lib, monkeypatch, capfd):
    """tests/golden/sac_plan_parent.json (tests/sac_plan_util.py): the plan dump with the tag sequence of every op list, the dump
    of connecting one rank (the exchange-closed lists), the variable table and the arena sizes of every shape of
    tests/test_hostemu_plan.py, the batch-16 shapes and the depth shape with each route switch moved alone: text byte for byte."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    gold = su.load_golden(os.path.join(GOLD, "sac_plan_parent.json"))
    cases = su.plan_cases()
    assert [c[0] for c in cases] == list(gold)
    for cid, switch, kw in cases:
        for k in su.SWITCH_VARS:
            monkeypatch.delenv(k, raising=False)
        if switch:
            monkeypatch.setenv(*switch)
        got = su.snapshot(kw, lambda: capfd.readouterr().err, hostemu_lib)
        want = gold[cid]
        for item in ("plan", "connect", "table", "sizes"):
            assert got[item] == want[item], (cid, item)
        assert "grl plan: seq ops_grads " in got["plan"] and "grl plan: seq ops_dp " in got["connect"], cid
