"""The launches of one training call of every plan on the g++ emulation build -- per tag: launches, FLOPs and bytes per launch --
and the exported host state, against tests/golden/launch_tags_parent.json: the parent's, byte for byte (tests/launch_tags_util.py
says how the file was written and what its cases reach)."""
import json
import os

import pytest

import launch_tags_util as lt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_tags_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(lt.CASES)
    return want


@pytest.mark.parametrize("name", list(lt.CASES))
def test_launches_and_state_are_the_parent_commits(hostemu_lib, monkeypatch, golden, name):
    monkeypatch.delenv("GRL_TUNE", raising=False)
    got = json.loads(json.dumps(lt.capture(name, hostemu_lib)))
    assert got["tags"] == golden[name]["tags"]
    assert got["state"] == golden[name]["state"]
