"""Host side of the VAE decoder's phase-decomposed upsample convs (`AutoEncoder.set_upsample`, SEVA_VAE_UPSAMPLE_PHASES,
`ops.conv3x3_up_phases128`; seva/_vae_engine.py): the switch, its environment default, which convs take the operator and with which
weights, and that a decode through a torch emulation of the four 2x2 phase convs matches the nine-tap decode to f16 weight
rounding.  Runs on tests/fake_ops.py, which has no `conv3x3_up_phases128`.  No GPU."""
import warnings

import pytest
import torch

import fake_ops
from conftest import rel_l2
from test_conv_upsample_phases_cpu import _phase_conv

SMALL = (64, 64, 128, 128)  # the decoder's topology, narrower: upsample convs with 128, 128 and 64 channels
UPS = [f"decoder.up_blocks.{i}.upsamplers.0.conv" for i in range(3)]


def _cpu(monkeypatch):
    from seva import _vae_engine
    monkeypatch.setattr(_vae_engine, "ops", fake_ops)
    monkeypatch.setattr(_vae_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_vae_engine.VaeDecoderEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))
    monkeypatch.delenv("SEVA_VAE_UPSAMPLE_PHASES", raising=False)
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    return _vae_engine


def _small_weights():
    from oracle import vae_ref as V
    from seva import synthetic as synth
    from seva.modules.autoencoder import VaeDecoderWeights
    wts = VaeDecoderWeights(block_out=SMALL)
    sd = synth.synth_state_dict(V.decoder_shapes(block_out=SMALL), 3)
    wts.load_state_dict(sd)
    return wts, sd


def _ae():
    from seva.modules.autoencoder import AutoEncoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return AutoEncoder(random_init=True)


def _spy_conv3x3(monkeypatch):
    seen = []
    real = fake_ops.conv3x3
    monkeypatch.setattr(fake_ops, "conv3x3", lambda x, w, **k: (seen.append(bool(k.get("upsample"))), real(x, w, **k))[1])
    return seen


def test_without_the_operator_phases_keeps_the_nine_tap_calls(monkeypatch):
    ve = _cpu(monkeypatch)
    assert not hasattr(fake_ops, "conv3x3_up_phases128")
    wts, _ = _small_weights()
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0)) * 0.18215 * 4
    want = ve.VaeDecoderEngine(wts).decode(z, 0.18215).clone()
    eng = ve.VaeDecoderEngine(wts, upsample="phases")
    seen = _spy_conv3x3(monkeypatch)
    got = eng.decode(z, 0.18215)
    assert sum(seen) == 3 and torch.equal(got, want)
    assert eng.W4 is None  # nothing packed for an operator that is not there


def test_phases_decode_takes_the_operator_with_combined_weights(monkeypatch):
    """With an operator of that name present, the 128-channel upsample convs take it with `.w4 == combine_up_phases(weight)`, the
    64-channel one keeps the nine taps; the decode differs from the nine-tap one by f16 weight rounding only (0 < rel-L2 < 1e-3,
    the UNet engine test's bound); "taps" afterwards gives the default bits again."""
    from seva._engine import combine_up_phases
    ve = _cpu(monkeypatch)
    wts, sd = _small_weights()
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1)) * 0.18215 * 4
    want = ve.VaeDecoderEngine(wts).decode(z, 0.18215).clone()
    calls = []

    def up_phases128(x16, w4, *, bias=None, out_f32=None, ch_stats=None, alg_k=0):
        calls.append((w4, alg_k, ch_stats is not None))
        n, ih, iw, cin = x16.shape
        r = _phase_conv(x16.permute(0, 3, 1, 2).float(), w4.float(), bias).permute(0, 2, 3, 1).reshape(n * 4 * ih * iw, -1)
        out_f32.view(r.shape).copy_(r)
        if ch_stats is not None:
            assert (ih * iw) % 64 == 0
            fake_ops._emit_stats(r, ch_stats)

    monkeypatch.setattr(fake_ops, "conv3x3_up_phases128", up_phases128, raising=False)
    eng = ve.VaeDecoderEngine(wts, upsample="phases")
    assert eng.W4 is None  # packed lazily
    seen = _spy_conv3x3(monkeypatch)
    got = eng.decode(z, 0.18215).clone()
    assert sum(seen) == 1 and len(calls) == 2  # up_blocks.2 has 64 channels: nine taps
    assert set(eng.W4) == {UPS[0] + ".w4", UPS[1] + ".w4"}
    for (w4, alg_k, _), p in zip(calls, UPS):
        assert alg_k == 9 * 128 and w4.dtype == torch.float16 and w4.shape == (4, 128, 4 * 128)
        assert torch.equal(w4, combine_up_phases(sd[p + ".weight"].float()))
    err = rel_l2(got, want)
    print(f"vae decode (emulated kernels), phases vs nine taps: rel-L2 {err:.3e}")
    assert 0 < err < 1e-3
    # switching back: the default bits, the operator untouched
    eng.upsample = "taps"
    del seen[:], calls[:]
    back = eng.decode(z, 0.18215)
    assert sum(seen) == 3 and not calls and torch.equal(back, want)
    # statistics reach the consumer where the engine asks producers for them at this size (gn_fused_stats = 2: every size)
    # and are used (fake_ops.groupnorm normalises with what it is handed): still the nine-tap decode to weight rounding
    eng.upsample, eng.gn_fused_stats = "taps", 2
    want2 = eng.decode(z, 0.18215).clone()
    eng.upsample = "phases"
    del calls[:]
    got2 = eng.decode(z, 0.18215)
    assert [c[2] for c in calls] == [True, True] and 0 < rel_l2(got2, want2) < 1e-3


def test_a_shape_the_kernel_does_not_tile_keeps_the_nine_taps(monkeypatch):
    """The per-image rule of the kernel, restated on the host: linear tiles while a 128-pixel tile's window fits 288 pixels, else
    16 x 8 source tiles."""
    from seva._vae_engine import up_phases128_applies
    for ih, iw in [(8, 8), (8, 72), (72, 72), (16, 144), (8, 96), (16, 16), (5, 7), (8, 24), (16, 48), (32, 96), (144, 144), (288, 288),
                   (96, 72), (192, 144)]:
        assert up_phases128_applies(ih, iw), (ih, iw)
    for ih, iw in [(8, 100), (72, 88), (12, 96), (1, 64)]:
        assert not up_phases128_applies(ih, iw), (ih, iw)


def test_set_upsample_validates_and_chains(monkeypatch):
    _cpu(monkeypatch)
    ae = _ae()
    assert ae.upsample == "taps"
    assert ae.set_upsample("phases") is ae and ae.upsample == "phases"
    assert ae.set_upsample("taps").upsample == "taps"
    for bad in ("nine", "PHASES", "", None, 1):
        with pytest.raises(ValueError):
            ae.set_upsample(bad)
    assert ae.upsample == "taps"  # a refused value changes nothing


def test_env_is_read_at_engine_build_and_the_method_wins(monkeypatch):
    from seva.modules.autoencoder import VaeWeights
    _cpu(monkeypatch)

    def small_ae():
        ae = _ae()
        ae.module = VaeWeights(block_out=SMALL).eval().requires_grad_(False)
        return ae

    ae = small_ae()
    monkeypatch.setenv("SEVA_VAE_UPSAMPLE_PHASES", "1")
    assert ae.upsample == "phases" and ae.engine().upsample == "phases"  # no set_upsample: the environment, at engine build
    monkeypatch.delenv("SEVA_VAE_UPSAMPLE_PHASES")
    assert ae.engine().upsample == "phases" and ae.upsample == "phases"  # read once
    ae.set_upsample("taps")
    assert ae.engine().upsample == "taps"  # the method reaches a built engine
    monkeypatch.setenv("SEVA_VAE_UPSAMPLE_PHASES", "1")
    ae = small_ae().set_upsample("taps")
    assert ae.upsample == "taps" and ae.engine().upsample == "taps"  # the method wins over the environment
    monkeypatch.setenv("SEVA_VAE_UPSAMPLE_PHASES", "0")
    ae = small_ae()
    assert ae.engine().upsample == "taps"
    assert ae.set_upsample("phases").engine().upsample == "phases"
