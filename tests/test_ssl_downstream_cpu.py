"""SimCLR downstream evaluation, the parts that need no GPU: the tower handles of a
MultiModalSimCLRModel and what downstream._source reads off them, LateFusionEncoder's widths
and errors, the drivers' signatures (the reference's parameter names and defaults,
training_structures/ssl_train.py), the performance-summary writer, and the host-side contract of
the fused eval-mode layer's C entry points."""
import inspect

import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def simclr():
    from avdino.models import MultiModalSimCLRModel
    return MultiModalSimCLRModel(output_dim=32, projection_dim=16, device="cpu", precision="32", seed=3)


def test_simclr_model_exposes_tower_handles(simclr):
    img, aud = simclr.image_encoder, simclr.audio_encoder
    assert (img.output_dim, img.modality, img.kind, img.prefix) == (32, "image", "image_simple", "image_encoder")
    assert (aud.output_dim, aud.modality, aud.kind, aud.prefix) == (32, "audio", "spectrogram_simple",
                                                                    "audio_encoder")
    assert img.act_dtype == aud.act_dtype == torch.float32
    # handles on the model's own store, not copies; the prefixes are spec.simclr_sd's
    assert img.store is simclr.store and aud.store is simclr.store
    assert "image_encoder.encoder.0.weight" in simclr.store.spec
    assert "audio_encoder.encoder.18.weight" in simclr.store.spec
    assert list(img.parameters())


def test_source_accepts_non_dino_encoders(simclr):
    from avdino.downstream import _probe_kwargs, _source
    from avdino.training_structures import LateFusionEncoder
    for h in (simclr.image_encoder, simclr.audio_encoder):
        store, kind, D, E, act, fd = _source(h, is_dino_based=False)
        assert store is simclr.store and kind == h.kind and D == 32 and E is None
        assert act == torch.float32 and fd == 0.0
        assert _probe_kwargs(h, False) == {"prefix": h.prefix}
    fus = LateFusionEncoder(simclr.audio_encoder, simclr.image_encoder)
    store, kind, D, E, act, _fd = _source(fus, is_dino_based=False)
    assert store is simclr.store and kind == "late_fusion_concat" and D == 64 and act == torch.float32
    assert _probe_kwargs(fus, False) == {
        "towers": [("image_simple", "image_encoder"), ("spectrogram_simple", "audio_encoder")],
        "fusion": "concat"}
    with pytest.raises(TypeError):
        _source(object(), is_dino_based=False)


def test_probe_copies_a_grouped_store(simclr):
    """The frozen copy keeps the source's arena layout (SimCLR lays its towers out in groups)."""
    from avdino.probe import LinearProbe
    probe = LinearProbe(simclr.store, "image_simple", 32, prefix="image_encoder")
    for k in simclr.store.spec:
        assert torch.equal(probe.store[k], simclr.store[k]), k
    assert probe.modality == "image" and probe.enc.enc.lins == ["image_encoder.encoder.14",
                                                               "image_encoder.projection.0"]
    two = LinearProbe(simclr.store, "late_fusion_concat", 64,
                      towers=[("image_simple", "image_encoder"), ("spectrogram_simple", "audio_encoder")])
    assert two.multimodal and not hasattr(two, "modality")
    with pytest.raises(ValueError):
        LinearProbe(simclr.store, "late_fusion_max", 64, fusion="max",
                    towers=[("image_simple", "image_encoder"), ("spectrogram_simple", "audio_encoder")])


class _Enc:
    def __init__(self, dim):
        self.output_dim = dim

    def parameters(self):
        return iter(())


def test_late_fusion_encoder_dims_and_errors():
    from avdino.training_structures import LateFusionEncoder
    assert LateFusionEncoder(_Enc(32), _Enc(48)).output_dim == 80
    assert LateFusionEncoder(_Enc(32), _Enc(48), fusion="concat").fusion == "concat"
    assert LateFusionEncoder(_Enc(32), _Enc(32), fusion="sum").output_dim == 32
    assert LateFusionEncoder(_Enc(32), _Enc(32), fusion="mean").output_dim == 32
    with pytest.raises(ValueError):
        LateFusionEncoder(_Enc(32), _Enc(48), fusion="sum")
    with pytest.raises(ValueError):
        LateFusionEncoder(_Enc(32), _Enc(48), fusion="mean")
    with pytest.raises(ValueError):
        LateFusionEncoder(_Enc(32), _Enc(32), fusion="max")
    with pytest.raises(NotImplementedError):
        LateFusionEncoder(_Enc(32), _Enc(32), proj_dim=64)
    sig = inspect.signature(LateFusionEncoder.__init__)
    assert list(sig.parameters) == ["self", "audio_encoder", "image_encoder", "fusion", "proj_dim"]
    assert sig.parameters["fusion"].default == "concat" and sig.parameters["proj_dim"].default is None


def test_drivers_have_the_reference_signatures():
    from avdino import training_structures as T
    sig = inspect.signature(T.train_and_evaluate_ssl)
    assert list(sig.parameters) == ["module", "train_data_module", "test_data_module", "model_dir",
                                    "model_name", "input_data", "modalities", "seeds", "num_epochs"]
    assert sig.parameters["modalities"].default == ["audio", "image"]
    assert sig.parameters["seeds"].default == [1, 2, 3]
    assert sig.parameters["num_epochs"].default == 100
    assert sig.parameters["input_data"].default is None
    sig = inspect.signature(T.evaluate_multimodal_ssl)
    assert list(sig.parameters) == ["lightning_cls", "ckpt_paths", "test_data_module", "model_name",
                                    "fusion", "proj_dim"]
    assert sig.parameters["fusion"].default == "concat" and sig.parameters["proj_dim"].default is None
    sig = inspect.signature(T.compute_train_results)
    assert list(sig.parameters) == ["pretrained_model", "model_path", "model_name", "traindata",
                                    "validdata", "testdata"]


def test_summary_writer_keys_and_format(tmp_path, simclr):
    from avdino.training_structures import ssl_model_stats, write_ssl_summary
    gflops, params = ssl_model_stats(simclr)
    assert params == sum(v.numel() for k, v in simclr.store.state_dict().items()
                         if simclr.store.spec[k][1] in ("w", "b", "bn_w", "bn_b"))
    assert gflops > 0
    path = tmp_path / "m_performance_summary.txt"
    perf = write_ssl_summary(str(path), "m", 1234567, 0.4567, [1, 2, 3], [3600.0, 7200.0, 5400.0],
                             {"image": ([90.0, 92.0, 94.0], [80.0, 80.0, 80.0]),
                              "audio": ([50.0, 51.0, 52.5], [40.25, 40.25, 40.25])})
    assert list(perf) == ["model_name", "parameters", "gflops", "seeds", "training_time_hours",
                          "downstream_mlp_acc_image", "downstream_knn_accuracy_image",
                          "downstream_mlp_acc_audio", "downstream_knn_accuracy_audio"]
    assert perf["parameters"] == "1.23M" and perf["gflops"] == "0.46"
    assert perf["training_time_hours"] == "1.50"
    assert perf["downstream_knn_accuracy_image"] == "92.0000 ± 1.6330"      # population std
    assert perf["downstream_mlp_acc_image"] == "80.0000 ± 0.0000"
    assert perf["downstream_mlp_acc_audio"] == "40.2500 ± 0.0000"
    lines = path.read_text().splitlines()
    assert lines == [f"{k}: {v}" for k, v in perf.items()]
    assert lines[3] == "seeds: [1, 2, 3]"
    only = write_ssl_summary(str(path), "m", 1, 0.0, [1], [1.0], {"audio": ([1.0], [2.0])})
    assert [k for k in only if k.startswith("downstream")] == ["downstream_mlp_acc_audio",
                                                               "downstream_knn_accuracy_audio"]


def test_csv_logger_string_version_is_the_directory(tmp_path):
    from avdino.trainer import CSVLogger
    lg = CSVLogger(str(tmp_path), name="logs", version="version_seed2")
    assert lg.log_dir == str(tmp_path / "logs" / "version_seed2")
    assert CSVLogger(str(tmp_path), name="logs", version=4).log_dir == str(tmp_path / "logs" / "version_4")


def test_c3_eval_host_contract():
    from avdino._lib import lib
    import ctypes
    d = ctypes.c_void_p(64)
    assert lib.avd_c3_conv_eval(None, None, None, None, None, None, 0, 2, 28, 28, 32, 64, None) == -4
    assert lib.avd_c3_conv_eval(d, d, None, d, None, d, 0, 2, 28, 28, 32, 64, None) == -4
    # shapes outside the table are declined (0), never an error; nothing is launched
    for shape in [(2, 28, 28, 8, 64, 0), (2, 28, 28, 32, 48, 0), (2, 64, 64, 32, 64, 0),
                  (2, 28, 28, 32, 512, 0), (2, 56, 56, 32, 64, 1), (2, 28, 28, 32, 64, 2),
                  (0, 28, 28, 32, 64, 0)]:
        assert lib.avd_c3_eval_serves(*shape) == 0, shape
        N, H, W, C, O, mode = shape
        assert lib.avd_c3_conv_eval(d, d, None, d, d, d, mode, N, H, W, C, O, None) == 0, shape
    # the SimCLR encoders' layers at a full and at a ragged evaluation batch
    for N in (128, 16, 5):
        for (H, C, O, mode) in [(56, 32, 64, 0), (28, 64, 128, 0), (14, 128, 256, 1), (14, 32, 64, 0),
                                (7, 64, 128, 1)]:
            assert lib.avd_c3_eval_serves(N, H, H, C, O, mode) == 1, (N, H, C, O, mode)
