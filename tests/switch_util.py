"""The `grl tune:` notes of GRL_PLAN_DUMP (csrc/engine.hip: Switches::note; the table of switches is README.md, "Switches"),
shared by the CPU test on the emulation build (tests/test_hostemu_switches.py) and the GPU case of tests/test_gpu_api.py."""
import re

import q_parity_util as qu

MIXED = "q_chain_late=0,bogus=1,fused_qapply=0"        # two keys of the table around one that is not


def tune_notes(dump):
    """(settings, unknown): the `key=value` items of every `grl tune: ...` line (one line per planning run that has a switch off
    its default: the dry run of grl_query_sizes and grl_create each plan once) and the key of every unknown-key line."""
    settings, unknown = [], []
    for line in dump.splitlines():
        if line.startswith("grl tune:"):
            m = re.fullmatch(r"grl tune: unknown key '(.*)' ignored", line)
            if m:
                unknown.append(m.group(1))
            else:
                settings.append(sorted(line.split()[2:]))
    return settings, unknown


def dqn_dump(monkeypatch, capfd, tune, backend=None, lib_path=None):
    """GRL_PLAN_DUMP text of creating the smallest DQN handle (CASES["dqn"] at B = 16) under GRL_TUNE=tune."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    monkeypatch.setenv("GRL_TUNE", tune)
    capfd.readouterr()
    case = qu.make_q_case(**qu.case_args("dqn", B=16))
    qu.QEngine(case["cfg"], backend=backend, lib_path=lib_path).close()
    return capfd.readouterr().err


def check_mixed_string(dump_of, matrix_cores):
    """MIXED: both known keys on every `grl tune:` line and nothing else, `bogus` -- and only it -- reported once per planning
    run, and `q_chain` (a prefix of `q_chain_late`) left at its default.  dump_of(tune) -> GRL_PLAN_DUMP text.

    The routes: `fused_qapply=0` itself takes the chained backward away (plan_q.inl: q_chain needs the fused apply launch), so the
    route under MIXED is compared with the one the same string gives without `bogus`, and `q_chain_late=0,bogus=1` with
    `q_chain_late=0` alone -- which still forms loss and weight gradients inside the backward chains: q_chain did not move."""
    dump = dump_of(MIXED)
    settings, unknown = tune_notes(dump)
    assert len(settings) >= 1 and all(s == ["fused_qapply=0", "q_chain_late=0"] for s in settings), dump
    assert unknown == ["bogus"] * len(settings), dump
    route = lambda text: qu.route_from_dump(text, matrix_cores=matrix_cores)
    assert route(dump) == route(dump_of("q_chain_late=0,fused_qapply=0"))
    late_only = route(dump_of("q_chain_late=0"))
    assert "chained" in late_only and route(dump_of("q_chain_late=0,bogus=1")) == late_only
    assert "chained" not in route(dump_of("q_chain=0"))
