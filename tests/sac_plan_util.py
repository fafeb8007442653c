"""The handles of tests/golden/sac_plan_parent.json: the nine shapes of tests/test_hostemu_plan.py, the batch-16 shapes that get
the "gather_ride" call plan, the vector-observation plan and the wide head kernel, and the depth shape at batch 16 with each
route switch moved alone -- and what is recorded of one: the GRL_PLAN_DUMP text of constructing it (launch notes and one
`grl plan: seq <list>  <tag> ...` line per op list), the text of grl_allreduce_init + grl_allreduce_connect with one rank, its
variable table and the arena sizes grl_query_sizes returns.  The file was written by
`python tests/sac_plan_util.py <emulation library> <out.json>` at the commit before csrc/plan_sac.inl was split into steps (with
only the `seq` lines added to it); tests/test_hostemu_sac_plan.py holds every later plan against it."""
import json
import os
import sys
import tempfile

if __name__ == "__main__":          # run as a script: the import paths tests/conftest.py sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "deep-rl-grasping_amd")]

import parity_util as pu
from hostemu_backend import NumpyHostBackend
from test_hostemu_plan import CASES

DEPTH16 = dict(extractor="augmented", kind="depth", B=16, n_replay=48)
SWITCHES = [("GRL_NO_HEADS_MFMA", "1"), ("GRL_NO_FUSED_HEADS", "1"), ("GRL_NO_V2", "1")] + \
           [("GRL_TUNE", t) for t in ("conv_stack=0", "conv_stack_bwd=1", "gather_prefetch=0", "gather_ride=0", "fused_adam=0", "l0_split=1", "store_drain=0")]
SWITCH_VARS = sorted({k for k, _ in SWITCHES})


def plan_cases():
    """[(id, (variable, value) or None, make_case arguments)]"""
    out = [("case/" + n, None, kw) for n, kw in CASES.items()]
    out.append(("b16/depth_augmented", None, DEPTH16))
    out.append(("b16/mlp", None, dict(extractor="mlp", B=16, n_replay=64)))
    out.append(("b16/layers_128_128", None, dict(DEPTH16, layers=(128, 128))))
    for k, v in SWITCHES:
        out.append(("switch/%s=%s" % (k, v), (k, v), DEPTH16))
    return out


def snapshot(kw, read_plan, lib_path):
    """What the golden file holds of one handle.  read_plan() returns the GRL_PLAN_DUMP text written since its last call."""
    case = pu.make_case(n_steps=1, **kw)
    read_plan()
    eng = pu.SacEngine(case["cfg"], backend=NumpyHostBackend(), lib_path=lib_path)
    try:
        plan = read_plan()
        eng.allreduce_connect([eng.allreduce_init(0, 1)])
        connect = read_plan()
        s = eng.sizes
        return {"plan": plan, "connect": connect,
                "table": [[name, off, list(shape), int(tr)] for name, off, _, shape, tr in eng.table],
                "sizes": {k: int(getattr(s, k)) for k in ("state_bytes", "grads_bytes", "work_bytes", "replay_bytes", "n_params", "n_trainable")}}
    finally:
        eng.close()


def load_golden(path):
    """{id: {"plan", "connect", "table", "sizes"}}; in the file the handles of one network share their table ("tables") and a
    text is the list of its lines' indices in "lines" (every line ends in a newline)."""
    doc = json.load(open(path))
    text = lambda ix: "".join(doc["lines"][i] + "\n" for i in ix)
    return {k: dict(v, table=doc["tables"][v["table"]], plan=text(v["plan"]), connect=text(v["connect"])) for k, v in doc["cases"].items()}


def stderr_reader():
    """Points file descriptor 2 at a temporary file; the returned read_plan() gives the text written since its last call."""
    err = tempfile.TemporaryFile()
    os.dup2(err.fileno(), 2)

    def read_plan():
        sys.stderr.flush()
        n = os.lseek(2, 0, os.SEEK_CUR)
        text = os.pread(2, n - read_plan.at, read_plan.at).decode()
        read_plan.at = n
        return text
    read_plan.at = 0
    return read_plan


def _record(lib_path, out_path):
    os.environ["GRL_PLAN_DUMP"] = "1"
    read_plan = stderr_reader()
    tables, lines, cases = [], [], {}

    def line_indices(text):
        assert text.endswith("\n")
        for ln in text[:-1].split("\n"):
            if ln not in lines:
                lines.append(ln)
        return [lines.index(ln) for ln in text[:-1].split("\n")]
    for cid, switch, kw in plan_cases():
        for k in SWITCH_VARS:
            os.environ.pop(k, None)
        if switch:
            os.environ[switch[0]] = switch[1]
        snap = snapshot(kw, read_plan, lib_path)
        if snap["table"] not in tables:
            tables.append(snap["table"])
        cases[cid] = dict(snap, table=tables.index(snap["table"]), plan=line_indices(snap["plan"]), connect=line_indices(snap["connect"]))
    with open(out_path, "w") as f:
        f.write('{"lines": ' + json.dumps(lines, indent=0) + ',\n"tables": [\n' + ",\n".join(json.dumps(t, separators=(",", ":")) for t in tables) + '\n],\n"cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in cases.items()) + "\n}}\n")


if __name__ == "__main__":
    _record(sys.argv[1], sys.argv[2])
