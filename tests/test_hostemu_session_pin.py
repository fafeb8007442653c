"""A behaviour-cloning session and a GAIL session on the g++ emulation build -- plan lines, launches per tag, every fetched result,
a second session on the same handle -- against tests/golden/session_parent.json: the parent's, bit for bit
(tests/session_pin_util.py says how the file was written and what a case records).  Every session runs in a buffer of exactly the
size its dry query returned, with guard words behind it that must stay untouched."""
import json
import os

import pytest

import session_pin_util as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "session_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(sp.CASES)
    return want


@pytest.mark.parametrize("name", sp.CASES)
def test_sessions_are_the_parent_commits(hostemu_lib, monkeypatch, golden, name):
    monkeypatch.delenv("GRL_TUNE", raising=False)
    got = json.loads(json.dumps(sp.capture(name, hostemu_lib)))
    for key in sorted(set(got) | set(golden[name])):      # (key by key: a failure names what moved)
        assert got.get(key) == golden[name].get(key), key
    assert got == golden[name]
