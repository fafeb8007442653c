"""Auto-encoder of any supported configuration (general launch plan, csrc/plan_ae.inl: plan_ae_general) on the CPU through the
TEST-ONLY g++ emulation build: every case of ae_general_util.CASES against the float32 restatement, the restatement against
oracle/autoencoder.py itself, which route a handle takes (plan dump), and what is refused."""
import ctypes as C

import numpy as np
import pytest

import ae_general_util as gu
from grasp_rl import _capi
from grasp_rl.autoencoder import PARAM_NAMES, SHIPPED_NET, SimpleAutoEncoder
from hostemu_backend import NumpyHostBackend
from oracle import autoencoder as oae


@pytest.mark.parametrize("net", [SHIPPED_NET, ((3, 3, 3), (8, 16, 32), 7, 0.1)], ids=["shipped", "k3_f8_16_32_dim7"])
def test_restatement_equals_the_oracle_bit_for_bit(net):
    """f2 = 32 and alpha = 0.1 are all AeOracle can express; there the restatement must BE the oracle."""
    B = 2
    P0, x = gu.case_inputs(net, B)
    a, b = gu.AeRestated(P0, alpha=0.1), oae.AeOracle(P0)
    for s in range(3):
        ra, rb = a.step(x[s * B:(s + 1) * B]), b.step(x[s * B:(s + 1) * B])
        assert ra["loss"] == rb["loss"] and np.array_equal(ra["out"], rb["out"]) and np.array_equal(ra["z"], rb["z"])
        assert all(np.array_equal(ra["grads"][k], rb["grads"][k]) for k in PARAM_NAMES)
    Pa, Pb = a.params(), b.params()
    assert all(np.array_equal(Pa[k], Pb[k]) for k in PARAM_NAMES)
    if net == SHIPPED_NET:      # (oae.encode reshapes nothing, but the module constant fixes the kernels it was written for)
        assert np.array_equal(a.encode(x[:3]), oae.encode(Pb, x[:3]))
    assert np.array_equal(a.reconstruct(x[:3]), b.forward(__import__("torch").from_numpy(x[:3]))[0].detach().numpy())


@pytest.mark.parametrize("name", list(gu.CASES))
def test_general_plan_matches_the_restatement(hostemu_lib, name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    gu.ae_general_check(name, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    ks, fs, dim, alpha, _ = gu.CASES[name]
    line = "grl plan: ae general   k=%d/%d/%d f=%d/%d/%d dim=%d alpha=%g\n" % (ks + fs + (dim, alpha))
    assert line in capfd.readouterr().err


def test_shipped_network_down_the_general_route(hostemu_lib, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    gu.shipped_general_check(monkeypatch, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    err = capfd.readouterr().err
    # two handles were built, each planned twice (size query + create): only the second handle took the general route
    assert err.count("grl plan: ae general   k=7/5/3 f=32/32/32 dim=100 alpha=0.1\n") == 2
    assert err.count("grl tune: ae_general=1") == 2


def test_shipped_configuration_keeps_the_tuned_route(hostemu_lib, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    monkeypatch.delenv("GRL_TUNE", raising=False)
    text = gu.plan_text_and_table(hostemu_lib, NumpyHostBackend(), capfd)
    assert "ae general" not in text and "ae_out_conv_bwd" in text
    # the shipped values written out reach the library as zeros: the same handle, the same route
    assert gu.plan_text_and_table(hostemu_lib, NumpyHostBackend(), capfd, net=SHIPPED_NET) == text


def _cfg(net):
    ks, fs, dim, alpha = net
    cfg = _capi.make_ae_config(4, 2e-4, 4)
    for i in range(3):
        cfg.ae_kernel[i], cfg.ae_filters[i] = ks[i], fs[i]
    cfg.ae_encoding_dim, cfg.ae_alpha = dim, alpha
    return cfg


def _layers(ks, fs, strides=(2, 2, 2)):
    return [{"filters": f, "kernel_size": k, "strides": s} for k, f, s in zip(ks, fs, strides)]


REFUSED = {
    "kernel_11": ((11, 5, 3), (32, 32, 32), 100, 0.1),
    "filters_6": ((7, 5, 3), (32, 6, 32), 100, 0.1),
    "filters_68": ((7, 5, 3), (68, 32, 32), 100, 0.1),
    "dim_0": ((7, 5, 3), (32, 32, 32), 0, 0.1),
    "dim_1025": ((7, 5, 3), (32, 32, 32), 1025, 0.1),
    "alpha_1": ((7, 5, 3), (32, 32, 32), 100, 1.0),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_sizes_outside_the_domain_are_refused(hostemu_lib, name):
    ks, fs, dim, alpha = REFUSED[name]
    with pytest.raises(NotImplementedError, match="kernel_size 1..9"):
        SimpleAutoEncoder({"network": _layers(ks, fs), "encoding_dim": dim, "alpha": alpha}, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    lib = _capi.load_library(hostemu_lib)
    sizes = _capi.GrlSizes()
    assert lib.grl_query_sizes(C.byref(_cfg(REFUSED[name])), C.byref(sizes)) == -1          # GRL_ERR_INVALID
    assert b"kernel_size 1..9" in lib.grl_last_error()
    bufs, h = _capi.GrlBuffers(), C.c_void_p()
    keep = [np.zeros(64, np.float32) for _ in range(4)]
    bufs.state, bufs.grads, bufs.work, bufs.replay = [k.ctypes.data for k in keep]
    assert lib.grl_create(C.byref(_cfg(REFUSED[name])), C.byref(bufs), C.byref(h)) == -1


def test_other_depths_and_strides_are_refused():
    four = _layers((7, 5, 3, 3), (32, 32, 32, 32), (2, 2, 2, 2))
    with pytest.raises(NotImplementedError, match="three encoder layers"):
        SimpleAutoEncoder({"network": four, "encoding_dim": 100})
    with pytest.raises(NotImplementedError, match="strides 2"):
        SimpleAutoEncoder({"network": _layers((7, 5, 3), (32, 32, 32), (2, 1, 2)), "encoding_dim": 100})


def test_ae_fields_on_a_sac_configuration_are_refused(hostemu_lib):
    lib = _capi.load_library(hostemu_lib)
    cfg = _capi.make_config("mlp", obs_dim=8, act_dim=2)
    sizes = _capi.GrlSizes()
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(sizes)) == 0
    cfg.ae_encoding_dim = 16
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(sizes)) == -1
    assert b"auto-encoder handles" in lib.grl_last_error()
    cfg.ae_encoding_dim, cfg.ae_alpha = 0, 0.3
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(sizes)) == -1


def test_state_blobs_keep_their_hash_and_the_shorter_struct_still_imports(hostemu_lib):
    """The ae_* fields stay out of the configuration hash while they are zero, and a blob that holds the grl_config as it was
    before they were appended (32 bytes shorter) is accepted: they read as zeros, the shipped network."""
    from grasp_rl.autoencoder import AeEngine
    eng = AeEngine(2, 2e-4, act_batch=2, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    blob = bytes(eng.export_state())
    hdr = _capi.GrlStateHeader.from_buffer_copy(blob[:C.sizeof(_capi.GrlStateHeader)])
    hsz, csz = C.sizeof(_capi.GrlStateHeader), C.sizeof(_capi.GrlConfig)
    assert hdr.config_bytes == csz and _capi.GrlConfig.ae_kernel.offset == csz - 32
    assert hdr.config_hash == 0xdc13959072e0372f         # what the commit before the fields printed for this configuration
    # FNV-1a over the fields in order, as before the fields existed (checkpoint.inl): the tail contributes nothing
    cfg = blob[hsz:hsz + csz]
    assert cfg[csz - 32:] == bytes(32)
    short = _capi.GrlStateHeader.from_buffer_copy(blob[:hsz])
    short.config_bytes, short.total_bytes = csz - 32, hdr.total_bytes - 32
    eng.import_state(bytes(short) + blob[hsz:hsz + csz - 32] + blob[hsz + csz:])
    eng.import_state(blob)
    eng.close()
    other = AeEngine(2, 2e-4, act_batch=2, backend=NumpyHostBackend(), lib_path=hostemu_lib, net=((3, 3, 3), (8, 16, 32), 7, 0.1))
    assert bytes(other.export_state())[:hsz] != blob[:hsz]          # another network: another hash
    with pytest.raises(_capi.GrlError, match="ae_kernel differs"):
        other.import_state(blob)
    other.close()
