"""Host side of the opt-in fp8 VAE encoder (seva/_vae_engine.py, AutoEncoder.set_precision(..., encode=)): the encode precision
switch, its environment default, which encoder convs the packer quantises, how close their e4m3 weights are to the originals, and
which convs the encoder issues in e4m3 (HIP operators emulated by tests/fake_ops.py).  No GPU work happens here."""
import warnings

import pytest
import torch

SD21 = (128, 256, 512, 512)

# every resnet 3x3 conv of the encoder with cin % 128 == 0 and cout % 128 == 0, except conv2 of the two channel-changing resnets
# (down_blocks.1.resnets.0: 128 -> 256, down_blocks.2.resnets.0: 256 -> 512), whose folded 1x1 shortcut is f16-only
EXPECTED = (
    [f"encoder.down_blocks.0.resnets.{j}.conv{c}" for j in (0, 1) for c in (1, 2)]
    + ["encoder.down_blocks.1.resnets.0.conv1"] + [f"encoder.down_blocks.1.resnets.1.conv{c}" for c in (1, 2)]
    + ["encoder.down_blocks.2.resnets.0.conv1"] + [f"encoder.down_blocks.2.resnets.1.conv{c}" for c in (1, 2)]
    + [f"encoder.down_blocks.3.resnets.{j}.conv{c}" for j in (0, 1) for c in (1, 2)]
    + [f"encoder.mid_block.resnets.{r}.conv{c}" for r in (0, 1) for c in (1, 2)]
)
# ... and, with SEVA_VAE_FP8_DOWNSAMPLE=1 only, the three downsample convs
DOWNSAMPLERS = [f"encoder.down_blocks.{i}.downsamplers.0.conv" for i in (0, 1, 2)]


def _ae():
    from seva.modules.autoencoder import AutoEncoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return AutoEncoder(random_init=True)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ("SEVA_VAE_PRECISION", "SEVA_VAE_ENCODE_PRECISION", "SEVA_VAE_FP8_DOWNSAMPLE"):
        monkeypatch.delenv(k, raising=False)


def test_encode_argument_is_validated_and_chains():
    ae = _ae()
    assert ae.encode_precision == "f16"
    assert ae.set_precision("f16", encode="fp8") is ae and (ae.precision, ae.encode_precision) == ("f16", "fp8")
    assert ae.set_precision("fp8", encode="f16").encode_precision == "f16" and ae.precision == "fp8"
    assert ae.set_precision("f16").encode_precision == "f16"  # encode=None leaves it as it is
    ae.set_precision("f16", encode="fp8")
    assert ae.set_precision("fp8").encode_precision == "fp8" and ae.precision == "fp8"
    for bad in ("bf16", "FP8", "e4m3", ""):
        with pytest.raises(ValueError):
            ae.set_precision("f16", encode=bad)
        with pytest.raises(ValueError):
            ae.set_precision(bad, encode="f16")
    assert (ae.precision, ae.encode_precision) == ("fp8", "fp8")  # a refused value changes nothing, on either side


def test_decode_switch_alone_leaves_encode_f16():
    ae = _ae().set_precision("fp8")
    assert (ae.precision, ae.encode_precision) == ("fp8", "f16")


def test_env_default_and_precedence(monkeypatch):
    monkeypatch.setenv("SEVA_VAE_ENCODE_PRECISION", "fp8")
    ae = _ae()
    assert (ae.precision, ae.encode_precision) == ("f16", "fp8")  # no encode=: the environment decides, decode untouched
    assert ae.set_precision("fp8").encode_precision == "fp8"
    assert ae.set_precision("fp8", encode="f16").encode_precision == "f16"  # encode= wins over the environment
    monkeypatch.setenv("SEVA_VAE_ENCODE_PRECISION", "f16")
    monkeypatch.setenv("SEVA_VAE_PRECISION", "fp8")
    ae = _ae()
    assert (ae.precision, ae.encode_precision) == ("fp8", "f16")  # the two variables are independent
    assert ae.set_precision("f16", encode="fp8").encode_precision == "fp8"
    monkeypatch.setenv("SEVA_VAE_ENCODE_PRECISION", "int8")
    with pytest.raises(ValueError):
        _ae().encode_precision
    assert _ae().set_precision("f16", encode="f16").encode_precision == "f16"  # an explicit choice never reads the (bad) variable


def test_unet_precision_switch_does_not_touch_the_encoder(monkeypatch):
    monkeypatch.setenv("SEVA_PRECISION", "fp8")
    monkeypatch.setenv("SEVA_FP8_ATTENTION", "1")
    assert _ae().encode_precision == "f16"


def test_quantised_encoder_set_is_exactly_the_listed_one(monkeypatch):
    from seva._vae_engine import fp8_downsample_from_env, fp8_encoder_convs, pack_fp8_convs
    names = fp8_encoder_convs(SD21)
    assert sorted(names) == sorted(EXPECTED) and len(names) == len(set(names)) == 18
    assert sorted(fp8_encoder_convs(SD21, downsample=True)) == sorted(EXPECTED + DOWNSAMPLERS)
    ae = _ae()
    sd = ae.module.state_dict()
    for dn, want in ((False, EXPECTED), (True, EXPECTED + DOWNSAMPLERS)):
        W8 = pack_fp8_convs(sd, ae.module.block_out, names=fp8_encoder_convs(ae.module.block_out, dn))
        assert set(W8) == {p + s for p in want for s in (".w8", ".w8e")}
        stay_f16 = ["quant_conv", "encoder.conv_in", "encoder.conv_out", "encoder.down_blocks.1.resnets.0.conv2",
                    "encoder.down_blocks.2.resnets.0.conv2"] + [f"encoder.mid_block.attentions.0.{n}" for n in ("to_q", "to_k", "to_v", "to_out.0")]
        for p in stay_f16 + ([] if dn else DOWNSAMPLERS):
            assert p + ".weight" in sd and not any(k.startswith(p + ".") for k in W8), p
        assert not any(k.startswith("decoder.") for k in W8)
    assert not fp8_downsample_from_env()
    monkeypatch.setenv("SEVA_VAE_FP8_DOWNSAMPLE", "1")
    assert fp8_downsample_from_env()


def test_narrow_topology_quantises_only_128k_channel_convs():
    from seva._vae_engine import fp8_encoder_convs
    names = fp8_encoder_convs((64, 64, 128, 128), downsample=True)
    assert sorted(names) == sorted([f"encoder.down_blocks.2.resnets.1.conv{c}" for c in (1, 2)]
                                   + [f"encoder.down_blocks.3.resnets.{j}.conv{c}" for j in (0, 1) for c in (1, 2)]
                                   + [f"encoder.mid_block.resnets.{r}.conv{c}" for r in (0, 1) for c in (1, 2)]
                                   + ["encoder.down_blocks.2.downsamplers.0.conv"])


def test_dequantised_encoder_weights_are_within_e4m3_rounding():
    from seva import ops
    from seva._vae_engine import fp8_encoder_convs, pack_fp8_convs
    ae = _ae()
    sd = ae.module.state_dict()
    W8 = pack_fp8_convs(sd, ae.module.block_out, names=fp8_encoder_convs(ae.module.block_out, downsample=True))
    for k in [k for k in W8 if k.endswith(".w8")]:
        p = k[: -len(".w8")]
        w = sd[p + ".weight"].float()
        cout, cin = w.shape[:2]
        rows = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        w8, e8 = W8[k], W8[k + "e"]
        assert w8.dtype == e8.dtype == torch.uint8 and w8.shape == (cout, 9 * cin) and e8.shape == (cout,)
        scale = torch.exp2(e8.float() - 127.0)[:, None]
        deq = ops.dequantize_weight_fp8(w8, e8)
        assert torch.equal(deq, (rows / scale).to(torch.float8_e4m3fn).float() * scale), p
        amax = (rows / scale).abs().amax(1)
        assert bool(((amax > 224.0) & (amax <= 448.0)).all()), p
        ulp = torch.maximum(torch.exp2(torch.floor(torch.log2((rows / scale).abs().clamp_min(2.0 ** -6))) - 3), torch.tensor(2.0 ** -9))
        assert bool(((deq - rows).abs() <= 0.5 * ulp * scale).all()), p


def _fake_encoder(monkeypatch, calls):
    """VaeEncoderEngine on the CPU with fake_ops; conv3x3 records (weight key, e4m3?, stride) and emulates out_f8 (saturating RNE)."""
    import fake_ops
    from seva import _vae_engine

    class Ops:
        pass

    ops = Ops()
    ops.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})

    def conv3x3(x, w, *, out_f8=None, out_f32=None, **kw):
        calls.append((id(w), kw.get("w_exp") is not None, kw.get("stride", 1), out_f8 is not None))
        if out_f8 is not None:
            tmp = torch.empty(out_f8.shape, dtype=torch.float32)
            fake_ops.conv3x3(x, w, out_f32=tmp, **kw)
            out_f8.copy_(fake_ops.to_fp8(tmp))
            if out_f32 is not None:
                out_f32.copy_(tmp)
            return
        fake_ops.conv3x3(x, w, out_f32=out_f32, **kw)

    ops.conv3x3 = conv3x3
    monkeypatch.setattr(_vae_engine, "ops", ops)
    monkeypatch.setattr(_vae_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_vae_engine.VaeEncoderEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))


@pytest.mark.parametrize("downsample", [False, True])
def test_encoder_issues_e4m3_convs_for_exactly_the_listed_convs(monkeypatch, downsample):
    from oracle import vae_ref as V
    from seva import _vae_engine, synthetic as synth
    from seva.modules.autoencoder import VaeWeights
    calls = []
    _fake_encoder(monkeypatch, calls)
    if downsample:
        monkeypatch.setenv("SEVA_VAE_FP8_DOWNSAMPLE", "1")
    small = (128, 128, 256, 256)
    wts = VaeWeights(block_out=small)
    wts.load_state_dict(synth.synth_state_dict({**V.decoder_shapes(block_out=small), **V.encoder_shapes(block_out=small)}, 5))
    eng = _vae_engine.VaeEncoderEngine(wts, precision="fp8")
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1
    out = eng.encode(x, 0.18215)
    assert out.shape == (1, 4, 4, 4) and torch.isfinite(out).all()
    want = _vae_engine.fp8_encoder_convs(small, downsample)
    by_id = {id(v): k[: -len(".w8")] for k, v in eng.W8.items() if k.endswith(".w8")}
    e4m3 = [by_id[i] for i, f8, _, _ in calls if f8]
    assert sorted(e4m3) == sorted(want) and len(e4m3) == len(set(e4m3))
    assert all((s == 2) == (by_id[i].endswith("downsamplers.0.conv")) for i, f8, s, _ in calls if f8)
    # with the knob, the resnet in front of each e4m3 downsample conv writes that conv's operand as e4m3 bytes
    assert sum(o8 for *_, o8 in calls) == (3 if downsample else 0)
    assert sum(1 for _, f8, s, _ in calls if s == 2 and not f8) == (0 if downsample else 3)
    eng.precision = "f16"
    calls.clear()
    eng.encode(x, 0.18215)
    assert not any(f8 for _, f8, _, _ in calls)
