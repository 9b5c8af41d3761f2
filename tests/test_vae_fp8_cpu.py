"""Host side of the opt-in fp8 VAE decoder (seva/_vae_engine.py, AutoEncoder.set_precision): the precision switch, its
environment default, which decoder convs the packer quantises, and how close their e4m3 weights are to the originals.
No GPU work happens here."""
import warnings

import pytest
import torch

SD21 = (128, 256, 512, 512)

# every resnet 3x3 conv of the decoder with cin % 128 == 0 and cout % 128 == 0, except conv2 of the two channel-changing resnets
# (up_blocks.2.resnets.0: 512 -> 256, up_blocks.3.resnets.0: 256 -> 128), whose folded 1x1 shortcut is f16-only
EXPECTED = (
    [f"decoder.mid_block.resnets.{r}.conv{c}" for r in (0, 1) for c in (1, 2)]
    + [f"decoder.up_blocks.{i}.resnets.{j}.conv{c}" for i in (0, 1) for j in (0, 1, 2) for c in (1, 2)]
    + ["decoder.up_blocks.2.resnets.0.conv1"] + [f"decoder.up_blocks.2.resnets.{j}.conv{c}" for j in (1, 2) for c in (1, 2)]
    + ["decoder.up_blocks.3.resnets.0.conv1"] + [f"decoder.up_blocks.3.resnets.{j}.conv{c}" for j in (1, 2) for c in (1, 2)]
)
# ... and, with SEVA_VAE_FP8_UPSAMPLE=1 only, the three upsample convs
UPSAMPLERS = [f"decoder.up_blocks.{i}.upsamplers.0.conv" for i in (0, 1, 2)]


def _ae():
    from seva.modules.autoencoder import AutoEncoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return AutoEncoder(random_init=True)


def test_default_autoencoder_reports_f16(monkeypatch):
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    assert _ae().precision == "f16"


def test_set_precision_validates_and_chains(monkeypatch):
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    ae = _ae()
    assert ae.set_precision("fp8") is ae and ae.precision == "fp8"
    assert ae.set_precision("f16").precision == "f16"
    for bad in ("bf16", "FP8", "e4m3", "", None):
        with pytest.raises(ValueError):
            ae.set_precision(bad)
    assert ae.precision == "f16"  # a refused value changes nothing


def test_env_default_and_precedence(monkeypatch):
    monkeypatch.setenv("SEVA_VAE_PRECISION", "fp8")
    ae = _ae()
    assert ae.precision == "fp8"  # no set_precision: the environment decides
    ae.set_precision("f16")
    assert ae.precision == "f16"  # set_precision wins over the environment
    monkeypatch.setenv("SEVA_VAE_PRECISION", "f16")
    assert _ae().set_precision("fp8").precision == "fp8"
    monkeypatch.setenv("SEVA_VAE_PRECISION", "int8")
    with pytest.raises(ValueError):
        _ae().precision
    assert _ae().set_precision("f16").precision == "f16"  # an explicit choice never reads the (bad) variable


def test_unet_precision_switch_does_not_touch_the_vae(monkeypatch):
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_PRECISION", "fp8")
    monkeypatch.setenv("SEVA_FP8_ATTENTION", "1")
    assert _ae().precision == "f16"


def test_quantised_conv_set_is_exactly_the_listed_one(monkeypatch):
    from seva._vae_engine import fp8_decoder_convs, fp8_upsample_from_env, pack_fp8_convs
    names = fp8_decoder_convs(SD21)
    assert sorted(names) == sorted(EXPECTED) and len(names) == len(set(names)) == 26
    assert sorted(fp8_decoder_convs(SD21, upsample=True)) == sorted(EXPECTED + UPSAMPLERS)
    ae = _ae()
    sd = ae.module.state_dict()
    for up, want in ((False, EXPECTED), (True, EXPECTED + UPSAMPLERS)):
        W8 = pack_fp8_convs(sd, ae.module.block_out, up)
        assert set(W8) == {p + s for p in want for s in (".w8", ".w8e")}
        stay_f16 = ["post_quant_conv", "decoder.conv_in", "decoder.conv_out", "decoder.up_blocks.2.resnets.0.conv2",
                    "decoder.up_blocks.3.resnets.0.conv2"] + [f"decoder.mid_block.attentions.0.{n}" for n in ("to_q", "to_k", "to_v", "to_out.0")]
        for p in stay_f16 + ([] if up else UPSAMPLERS):
            assert p + ".weight" in sd and not any(k.startswith(p + ".") for k in W8), p
        assert not any(k.startswith("encoder.") for k in W8)
    monkeypatch.delenv("SEVA_VAE_FP8_UPSAMPLE", raising=False)
    assert not fp8_upsample_from_env()
    monkeypatch.setenv("SEVA_VAE_FP8_UPSAMPLE", "1")
    assert fp8_upsample_from_env()


def test_narrow_topology_quantises_only_128k_channel_convs():
    from seva._vae_engine import fp8_decoder_convs
    names = fp8_decoder_convs((64, 64, 128, 128), upsample=True)
    assert sorted(names) == sorted([f"decoder.mid_block.resnets.{r}.conv{c}" for r in (0, 1) for c in (1, 2)]
                                   + [f"decoder.up_blocks.{i}.resnets.{j}.conv{c}" for i in (0, 1) for j in (0, 1, 2) for c in (1, 2)]
                                   + ["decoder.up_blocks.0.upsamplers.0.conv", "decoder.up_blocks.1.upsamplers.0.conv"])


def test_dequantised_weights_are_within_e4m3_rounding():
    """Each packed conv is the (ky, kx, ci)-ordered weight row scaled by a power of two and cast by torch's own e4m3 cast:
    de-quantised, it equals float8_e4m3fn(w * 2^-e) * 2^e exactly, and the scale puts each row's max in e4m3's top binade."""
    from seva import ops
    from seva._vae_engine import pack_fp8_convs
    ae = _ae()
    sd = ae.module.state_dict()
    W8 = pack_fp8_convs(sd, ae.module.block_out, upsample=True)
    for k in [k for k in W8 if k.endswith(".w8")]:
        p = k[: -len(".w8")]
        w = sd[p + ".weight"].float()
        cout, cin = w.shape[:2]
        rows = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        w8, e8 = W8[k], W8[k + "e"]
        assert w8.dtype == e8.dtype == torch.uint8 and w8.shape == (cout, 9 * cin) and e8.shape == (cout,)
        scale = torch.exp2(e8.float() - 127.0)[:, None]
        deq = ops.dequantize_weight_fp8(w8, e8)
        want = (rows / scale).to(torch.float8_e4m3fn).float() * scale
        assert torch.equal(deq, want), p
        amax = (rows / scale).abs().amax(1)
        assert bool(((amax > 224.0) & (amax <= 448.0)).all()), p
        # half an e4m3 ulp (3 mantissa bits) of each element, with the subnormal step 2^-9 of the scaled value as the floor
        ulp = torch.maximum(torch.exp2(torch.floor(torch.log2((rows / scale).abs().clamp_min(2.0 ** -6))) - 3), torch.tensor(2.0 ** -9))
        assert bool(((deq - rows).abs() <= 0.5 * ulp * scale).all()), p
