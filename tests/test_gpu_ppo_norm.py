"""VecNormalize observation statistics on PPO2 / TRPO handles on the MI355X: ppo_observe_kernel and the C ABI around it against
RunningMeanStd.update and VecNormalize.normalize_obs on the host, bit for bit (bodies and shapes: tests/ppo_norm_util.py, which
tests/test_hostemu_ppo_norm.py runs on the emulation build)."""
import pytest

import ppo_norm_util as nu
from grasp_rl.engine import PpoEngine, TrpoEngine

pytestmark = pytest.mark.gpu


@pytest.fixture
def dump(monkeypatch):
    monkeypatch.delenv("GRL_TUNE", raising=False)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")


def make(kind, obs_dim, n, normalize, n_steps=nu.N_CALLS):
    cfg, second = nu.engine_config(kind, obs_dim, n, normalize, n_steps=n_steps)
    eng = (PpoEngine if kind == "ppo" else TrpoEngine)(cfg, second)
    eng.set_parameters(nu.init_params(obs_dim))
    return eng


@pytest.mark.parametrize("kind,obs_dim,n", nu.OBSERVE_CASES)
def test_observe_is_the_hosts_update_and_normalize(dump, capfd, kind, obs_dim, n):
    nu.check_observe(make, lambda: capfd.readouterr().err, kind, obs_dim, n)


def test_what_the_handles_refuse(dump):
    from grasp_rl import _capi
    nu.check_refusals(make, _capi.load_library())


@pytest.mark.parametrize("kind", ["ppo", "trpo"])
def test_a_normalize_2_handle_on_the_host_path_is_a_normalize_0_handle(dump, kind):
    nu.check_host_path_unchanged(make, kind)
