"""`SimpleAutoEncoder` on a configuration other than the shipped one, end to end on the CPU (emulation build): train, save
model.h5 + model.npz, load into a fresh instance, encode the same bits; weights of another shape are refused by name."""
import numpy as np
import pytest

from grasp_rl import autoencoder
from grasp_rl.autoencoder import DeferredEncoder, PARAM_NAMES, SimpleAutoEncoder, glorot_uniform_params
from hostemu_backend import NumpyHostBackend

CONFIG = {"network": [{"filters": 16, "kernel_size": 5, "strides": 2}, {"filters": 16, "kernel_size": 3, "strides": 2},
                      {"filters": 32, "kernel_size": 3, "strides": 2}],
          "encoding_dim": 16, "learning_rate": 2e-4}


def _images(n, seed=3):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 64, 64, 1), np.float32)
    for i in range(n):
        r0, c0 = rng.integers(5, 40, 2)
        x[i, r0:r0 + 20, c0:c0 + 18, 0] = rng.uniform(0.2, 0.5, (20, 18))
    return x


def test_train_save_load_encode_on_a_configured_network(hostemu_lib, tmp_path):
    mk = lambda: SimpleAutoEncoder(CONFIG, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    model = mk()
    assert model.encoding_shape == (16,)
    x = _images(16)
    hist = model.train(x, x, batch_size=4, epochs=1, model_dir=str(tmp_path), validation_split=0.0)
    assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"][0])
    z = model.encode(x[:5])
    assert z.shape == (5, 16)
    w = model.get_weights()
    assert w["encoder/dense_1/kernel"].shape == (2048, 16) and w["decoder/conv2d_6/kernel"].shape == (5, 5, 16, 1)
    for name in ("model.h5", "model.npz"):
        assert (tmp_path / name).exists()
    fresh = mk()
    fresh.load_weights(str(tmp_path))            # model.h5
    assert np.array_equal(fresh.encode(x[:5]), z)
    (tmp_path / "model.h5").unlink()
    again = mk()
    again.load_weights(str(tmp_path))            # model.npz
    assert np.array_equal(again.encode(x[:5]), z)
    deferred = DeferredEncoder(CONFIG)
    autoencoder._DEFERRED.remove(deferred._record)       # (this process is no env worker: leave no record for a later fork to inherit)
    assert deferred.encoded_shape == model.encoding_shape
    for m in (model, fresh, again):
        m.engine.close()


def test_weights_of_the_shipped_shape_are_refused_by_name(hostemu_lib, tmp_path):
    shipped = SimpleAutoEncoder({"network": [{"filters": 32, "kernel_size": k, "strides": 2} for k in (7, 5, 3)], "encoding_dim": 100},
                                backend=NumpyHostBackend(), lib_path=hostemu_lib)
    shipped.save_weights(str(tmp_path))          # (no engine needed: the initial weights)
    model = SimpleAutoEncoder(CONFIG, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    with pytest.raises(ValueError, match="encoder/conv2d_1/kernel has shape \\(7, 7, 1, 32\\)"):
        model.load_weights(str(tmp_path))
    assert set(glorot_uniform_params(0)) == set(PARAM_NAMES)
