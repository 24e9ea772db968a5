"""-m "not gpu": N6, the opt-in Vocos decoder (ConvNeXt backbone + ISTFT head) on the host side -- presets, the
synthetic weights, the device pack, the inverse-DFT basis, the importer and the C ABI export.  The float64 reference below is plain
torch (F.conv1d / F.layer_norm / F.linear / F.gelu / torch.istft) and calls no product code; test_vocos_gpu.py checks the kernels
against it.  PARITY UNPINNED against the real decode graph (it cannot be fetched)."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import onnx_fixture_writer as ow
from vietvoice_tts_amd import onnx_import as oi
from vietvoice_tts_amd import pack
from vietvoice_tts_amd.model_pack import spec_by_name
from vietvoice_tts_amd.model_spec import ModelSpec, count_params, make_synthetic_weights, weight_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vocos_reference(spec, w, mel: torch.Tensor) -> torch.Tensor:
    """Float64 Vocos decoder: mel [T][n_mel] -> waveform [hop * (T - 1)] (torch.istft, centre padding, periodic Hann)."""
    d = lambda t: t.to(torch.float64)
    V, eps = spec.vocos_dim, spec.vocos_ln_eps
    h = F.conv1d(mel.to(torch.float64).T[None], d(w["voc.embed.weight"]), d(w["voc.embed.bias"]), padding=spec.vocos_embed_k // 2)[0].T
    h = F.layer_norm(h, (V,), d(w["voc.norm.weight"]), d(w["voc.norm.bias"]), eps)
    for i in range(spec.vocos_layers):
        p = f"voc.blocks.{i}"
        t = F.conv1d(h.T[None], d(w[p + ".dwconv.weight"]), d(w[p + ".dwconv.bias"]), padding=spec.vocos_dw_k // 2, groups=V)[0].T
        t = F.layer_norm(t, (V,), d(w[p + ".norm.weight"]), d(w[p + ".norm.bias"]), eps)
        t = F.gelu(F.linear(t, d(w[p + ".pwconv1.weight"]), d(w[p + ".pwconv1.bias"])))
        h = h + d(w[p + ".gamma"]) * F.linear(t, d(w[p + ".pwconv2.weight"]), d(w[p + ".pwconv2.bias"]))
    h = F.layer_norm(h, (V,), d(w["voc.final_norm.weight"]), d(w["voc.final_norm.bias"]), eps)
    return istft_reference(spec, F.linear(h, d(w["voc.head.weight"]), d(w["voc.head.bias"])))


def istft_reference(spec, o: torch.Tensor) -> torch.Tensor:
    """Head output [T][n_fft + 2] -> waveform [hop * (T - 1)], float64."""
    o = o.to(torch.float64)
    nb = spec.n_fft // 2 + 1
    if o.shape[0] < 2:
        return torch.zeros(0, dtype=torch.float64)
    mag = torch.exp(o[:, :nb]).clamp(max=100.0)
    S = torch.polar(mag, o[:, nb:]).T
    win = torch.hann_window(spec.win_length, periodic=True, dtype=torch.float64)
    return torch.istft(S, spec.n_fft, spec.hop_length, spec.win_length, win, center=True)


def reference_pcm(wave: torch.Tensor) -> torch.Tensor:
    return (wave * 32767.0).clamp(-32768.0, 32767.0).to(torch.int16)        # truncation toward zero


@pytest.mark.parametrize("name", ["tiny-vocos", "small-vocos", "full-vocos"])
def test_presets_and_json_round_trip(name):
    s = spec_by_name(name)
    base = spec_by_name(name[: -len("-vocos")])
    assert s.vocoder == "vocos" and base.vocoder == "hifigan"
    assert ModelSpec.from_json(s.to_json()) == s
    assert s.vocos_dim % 128 == 0 and s.vocos_intermediate % 128 == 0
    if name == "full-vocos":
        assert (s.vocos_dim, s.vocos_intermediate, s.vocos_layers, s.vocos_embed_k, s.vocos_dw_k) == (512, 1536, 8, 7, 7)
    assert s.pcm_samples(10) == 9 * s.hop_length and base.pcm_samples(10) == 10 * s.hop_length and s.pcm_samples(1) == 0


def test_old_spec_json_loads_as_hifigan():
    import json
    d = json.loads(ModelSpec.tiny().to_json())
    for k in [k for k in d if k == "vocoder" or k.startswith("vocos_")]:
        del d[k]
    s = ModelSpec.from_json(json.dumps(d))
    assert s == ModelSpec.tiny() and s.vocoder == "hifigan"


def test_acoustic_weights_identical_to_the_hifigan_preset():
    a, b = make_synthetic_weights(ModelSpec.tiny(), 9527), make_synthetic_weights(ModelSpec.tiny_vocos(), 9527)
    acoustic = [k for k in a if not k.startswith("voc.")]
    assert acoustic == [k for k in b if not k.startswith("voc.")]
    for k in acoustic:
        assert torch.equal(a[k], b[k]), k
    assert not any(k.startswith(("voc.pre", "voc.up", "voc.res", "voc.post")) for k in b)
    assert all(k.startswith("voc.") for k in b if k not in a)
    # every Vocos tensor counts as vocoder: ~13.5 M at full size (embed 0.36 M + 8 blocks x 1.58 M + head 0.53 M)
    n = count_params(ModelSpec.full_vocos())
    assert n["acoustic"] == count_params(ModelSpec.full())["acoustic"] and 13.0e6 < n["vocoder"] < 14.0e6


def test_pack_plan_holds_the_vocos_layouts():
    s = ModelSpec.tiny_vocos()
    for dt in (torch.float32, torch.bfloat16):
        es = {n: (d, shape) for n, d, shape, _fn in pack.entries(s, dt)}
        assert not any(n.startswith(("voc.pre", "voc.up", "voc.res", "voc.post")) for n in es)
        assert es["voc.embed.weight"] == (torch.float32, (s.vocos_dim, 704))
        assert es["voc.head.weight"] == (torch.float32, (1152, s.vocos_dim)) and es["voc.head.bias"] == (torch.float32, (1152,))
        assert es["voc.blocks.1.pwconv1.weight"] == (torch.float32, (s.vocos_intermediate, s.vocos_dim))
        assert es["voc.blocks.1.pwconv2.weight"] == (torch.float32, (s.vocos_dim, s.vocos_intermediate))
        assert es["voc.blocks.0.dwconv.weight"] == (torch.float32, (s.vocos_dim, 7))
        assert es["const.istft_basis"] == (torch.float32, (1024, 1024))
    w = make_synthetic_weights(s, 9527)
    fl = dict((n, fn(w)) for n, _d, _s, fn in pack.entries(s, torch.float32) if n.startswith("voc."))
    assert torch.equal(fl["voc.head.weight"][1026:], torch.zeros(126, s.vocos_dim)) and torch.equal(fl["voc.head.bias"][1026:], torch.zeros(126))
    # im2col order: column tap * n_mel + m
    we = w["voc.embed.weight"]
    assert torch.equal(fl["voc.embed.weight"][:, 3 * 100 + 17], we[:, 17, 3]) and torch.equal(fl["voc.embed.weight"][:, 700:], torch.zeros(s.vocos_dim, 4))
    # the HiFi-GAN plan is untouched by the new fields
    assert [n for n, *_ in pack.entries(ModelSpec.tiny(), torch.float32)][-1] == "voc.post.bias"


def test_istft_basis_is_the_windowed_inverse_real_dft():
    s = ModelSpec.full_vocos()
    basis = pack.istft_basis(s).to(torch.float64).numpy()
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, 513)) + 1j * rng.standard_normal((5, 513))
    operand = np.concatenate([X.real, X.imag[:, 1:512]], axis=1)             # Im of bins 0 and 512 are not inputs
    got = operand @ basis.T
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64).numpy()
    want = np.fft.irfft(X, 1024) * win
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def test_reference_peak_on_the_synthetic_weights():
    s = ModelSpec.small_vocos()
    w = make_synthetic_weights(s, 9527)
    mel = torch.randn(120, s.n_mel, generator=torch.Generator().manual_seed(0))
    y = vocos_reference(s, w, mel)
    assert y.shape == (s.hop_length * 119,)
    assert 0.1 <= float(y.abs().max()) <= 0.9


def _archive_models(spec, w):
    members = ow.export_archive_members(spec, w)
    return [oi.parse_model(members[k + ".onnx"]) for k in ("preprocess", "transformer", "decode")]


def test_importer_reads_a_vocos_decode_graph():
    s = ModelSpec.tiny_vocos()
    w = make_synthetic_weights(s, 9527)
    pre, tr, dec = _archive_models(s, w)
    names = set(oi.recover_names(dec))
    assert {"backbone.embed.weight", "backbone.convnext.1.gamma", "backbone.convnext.0.pwconv1.weight", "head.out.weight",
            "backbone.final_layer_norm.bias"} <= names
    assert not any(n.op_type == "ConvTranspose" for n in dec.nodes)
    spec, got = oi.import_graphs(pre, tr, dec, base=ModelSpec.tiny())
    assert spec == s
    assert set(got) == set(weight_shapes(s))
    for k, v in w.items():
        assert torch.equal(got[k], v), k


def test_importer_rejects_a_head_of_the_wrong_width():
    s = ModelSpec.tiny_vocos()
    w = make_synthetic_weights(s, 9527)
    pre, tr, _dec = _archive_models(s, w)
    V = s.vocos_dim
    inits = [(k, v.numpy(), "raw") for k, v in w.items() if k.startswith("voc.") and not k.startswith("voc.head")]
    inits = [(oi.exporter_names(k, 3)[0], a, how) for k, a, how in inits]
    inits += [("head.out.weight", np.zeros((1000, V), np.float32), "raw"), ("head.out.bias", np.zeros(1000, np.float32), "raw")]
    dec = oi.parse_model(ow.encode_model([], inits, [], []))
    with pytest.raises(oi.UnsupportedGraph, match="n_fft \\+ 2"):
        oi.import_graphs(pre, tr, dec, base=ModelSpec.tiny())


def test_graph_without_a_vocoder_still_says_no_convtranspose():
    s = ModelSpec.tiny()
    w = make_synthetic_weights(s, 9527)
    pre, tr, _dec = _archive_models(s, w)
    dec = oi.parse_model(ow.encode_model([oi.OnnxNode("Identity", "/id", ["denoised"], ["generated_signal"])], [], [], []))
    with pytest.raises(oi.UnsupportedGraph, match="no ConvTranspose"):
        oi.import_graphs(pre, tr, dec, base=ModelSpec.tiny())


def test_vv_set_vocos_is_declared_and_exported():
    from vietvoice_tts_amd import runtime as rt
    hdr = open(os.path.join(ROOT, "include", "vvtts.h")).read()
    for name in ("vv_set_vocos", "vv_istft_head", "vv_vocos_im2col"):
        assert re.search(r"VV_API int " + name + r"\(", hdr), name
        assert name in rt.EXPORTS
    assert re.search(r"typedef struct vv_vocos_cfg", hdr)
    assert [f for f, _ in rt.vv_vocos_cfg._fields_] == ["dim", "intermediate", "layers", "embed_k", "dw_k", "ln_eps", "n_fft", "win_length",
                                                        "hop_length"]
    assert re.search(r"#define VV_PROF_NCLASS 18", hdr)
    v = rt.vocos_cfg_from_spec(ModelSpec.full_vocos())
    assert (v.dim, v.intermediate, v.layers, v.n_fft, v.hop_length) == (512, 1536, 8, 1024, 256) and math.isclose(v.ln_eps, 1e-6, rel_tol=1e-6)
