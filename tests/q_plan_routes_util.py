"""The handles of tests/golden/q_plan_parent_routes.json: every shape, layer-norm and wide case of the DQN / BDQ tests, a
prioritised handle of either algorithm and the baseline BDQ shape with each route switch off -- and what is recorded of one:
the GRL_PLAN_DUMP text of constructing it, its variable table and the arena sizes grl_query_sizes returns.  The file was
written by `python tests/q_plan_routes_util.py <emulation library> <out.json>` at the commit before csrc/plan_q.inl was split
into steps; tests/test_hostemu_q_layer_norm.py holds every later plan against it."""
import json
import os
import sys
import tempfile

if __name__ == "__main__":          # run as a script: the import paths tests/conftest.py sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "deep-rl-grasping_amd")]

import q_layer_norm_util as lu
import q_parity_util as qu
import q_wide_util as qw
from grasp_rl.engine import QEngine
from hostemu_backend import NumpyHostBackend

SWITCHES_OFF = ("q_mfma", "q_l0_chain", "q_chain", "q_chain_late", "fused_qapply", "fused_q", "per_pf", "q_pf", "q_act")
EDGE_OBS = (2048, 2049)          # x 64 units: 131072 floats (not wide) and 131136 (wide)


def _prioritised(case, cap=3000):
    c = case["cfg"]
    c.replay_capacity = cap
    c.q_per, c.q_per_alpha, c.q_per_eps, c.q_per_alpha64 = 1, 0.6, 1e-6, 0.6
    return case


def route_cases():
    """[(id, GRL_TUNE, make_case)] -- make_case() returns a case of make_q_case's form (cfg, params, tr, ...)"""
    out = []
    for n in qu.SHAPE_CASES:
        out.append(("shape/" + n, "", lambda n=n: qu.make_q_case(**qu.case_args(n))))
    for n in lu.LN_CASES:
        out.append(("ln/" + n, "", lambda n=n: lu.make_ln_case(n)))
    for n in qw.PARITY_CASES:
        out.append(("wide/" + n, "", lambda n=n: qw.make_wide_case(n)))
    for d in EDGE_OBS:
        out.append(("wide/edge_%d" % d, "", lambda d=d: qw.make_wide_case("edge", obs_dim=d)))
    out.append(("per/bdq_baseline_config3", "", lambda: _prioritised(qu.make_q_case(**qu.case_args("bdq_baseline_config3", n_replay=300)))))
    out.append(("per/dqn_reference_shape", "", lambda: _prioritised(qu.make_q_case(**qu.case_args("dqn_reference_shape", n_replay=300)))))
    for s in SWITCHES_OFF:
        out.append(("switch/%s=0" % s, s + "=0", lambda: qu.make_q_case(**qu.case_args("bdq_baseline_config3"))))
    return out


def snapshot(case, read_plan, lib_path):
    """What the golden file holds of one handle.  read_plan() returns the GRL_PLAN_DUMP text written since its last call."""
    read_plan()
    eng = QEngine(case["cfg"], backend=NumpyHostBackend(), lib_path=lib_path)
    try:
        plan = read_plan()
        s = eng.sizes
        return {"plan": plan,
                "table": [[name, off, list(shape), int(tr)] for name, off, _, shape, tr in eng.table],
                "sizes": {k: int(getattr(s, k)) for k in ("state_bytes", "grads_bytes", "work_bytes", "replay_bytes", "n_params", "n_trainable")}}
    finally:
        eng.close()


def load_golden(path):
    """{id: {"tune", "plan", "table", "sizes"}}; in the file the handles of one network share their table ("tables") and a
    table names its variables by their index in the list "names".  """
    doc = json.load(open(path))
    tables = [[[doc["names"][r[0]]] + r[1:] for r in t] for t in doc["tables"]]
    return {k: dict(v, table=tables[v["table"]]) for k, v in doc["cases"].items()}


def _record(lib_path, out_path):
    os.environ["GRL_PLAN_DUMP"] = "1"
    err = tempfile.TemporaryFile()
    os.dup2(err.fileno(), 2)

    def read_plan():
        sys.stderr.flush()
        n = os.lseek(2, 0, os.SEEK_CUR)
        text = os.pread(2, n - read_plan.at, read_plan.at).decode()
        read_plan.at = n
        return text
    read_plan.at = 0
    tables, cases = [], {}
    for cid, tune, make in route_cases():
        os.environ.pop("GRL_TUNE", None)
        if tune:
            os.environ["GRL_TUNE"] = tune
        snap = snapshot(make(), read_plan, lib_path)
        if snap["table"] not in tables:
            tables.append(snap["table"])
        cases[cid] = {"tune": tune, "plan": snap["plan"], "table": tables.index(snap["table"]), "sizes": snap["sizes"]}
    names = sorted({r[0] for t in tables for r in t})
    tables = [[[names.index(r[0])] + r[1:] for r in t] for t in tables]
    with open(out_path, "w") as f:
        f.write('{"names": ' + json.dumps(names, indent=0) + ',\n"tables": [\n' + ",\n".join(json.dumps(t, separators=(",", ":")) for t in tables) + '\n],\n"cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in cases.items()) + "\n}}\n")


if __name__ == "__main__":
    _record(sys.argv[1], sys.argv[2])
