"""VecNormalize observation statistics on PPO2 / TRPO handles (grl_config.normalize = 2: grl_observe, ppo_observe_kernel, grl_ppo_step /
grl_ppo_finish with obs == NULL) through the C ABI on the g++ emulation build; the bodies are tests/ppo_norm_util.py's, which
tests/test_gpu_ppo_norm.py runs on the MI355X."""
import pytest

import ppo_norm_util as nu
from grasp_rl.engine import PpoEngine, TrpoEngine
from hostemu_backend import NumpyHostBackend


@pytest.fixture
def emu(hostemu_lib, monkeypatch):
    monkeypatch.delenv("GRL_TUNE", raising=False)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    return hostemu_lib


def _make(lib):
    def make(kind, obs_dim, n, normalize, n_steps=nu.N_CALLS):
        cfg, second = nu.engine_config(kind, obs_dim, n, normalize, n_steps=n_steps)
        eng = (PpoEngine if kind == "ppo" else TrpoEngine)(cfg, second, backend=NumpyHostBackend(), lib_path=lib)
        eng.set_parameters(nu.init_params(obs_dim))
        return eng
    return make


@pytest.mark.parametrize("kind,obs_dim,n", nu.OBSERVE_CASES)
def test_observe_is_the_hosts_update_and_normalize(emu, capfd, kind, obs_dim, n):
    nu.check_observe(_make(emu), lambda: capfd.readouterr().err, kind, obs_dim, n)


def test_what_the_handles_refuse(emu):
    from grasp_rl import _capi
    nu.check_refusals(_make(emu), _capi.load_library(emu))


def test_plan_and_sizes_without_normalize_are_the_parent_commits(emu, capfd):
    """tests/golden/ppo_plan_dump_parent.txt: GRL_PLAN_DUMP and the six numbers of grl_ppo_query_sizes / grl_trpo_query_sizes of
    normalize = 0 handles (two PPO shapes, one TRPO shape), captured from the parent commit on this build."""
    nu.check_plan_is_the_parents(lambda mod, c: mod.make_engine(c, backend=NumpyHostBackend(), lib_path=emu), lambda: capfd.readouterr().err)


@pytest.mark.parametrize("kind", ["ppo", "trpo"])
def test_a_normalize_2_handle_on_the_host_path_is_a_normalize_0_handle(emu, kind):
    nu.check_host_path_unchanged(_make(emu), kind)
