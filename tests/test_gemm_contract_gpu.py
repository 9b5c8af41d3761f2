"""The two promises of the GEMM / conv C-ABI (include/seva_hip.h) that the bit-equality claims of the project rest on.

A. Batch invariance.  A sample's result does not depend on the batch it is launched in: frame-sliced execution, the CFG split over
   two ranks and sharded == single-process all compare bits.  The dispatcher picks tile height, the A-in-registers variant, split-K,
   window vs per-tap gather and the window tiling from M = n * hw, so every case here runs a small launch and a large one whose
   leading rows / images are the same RANDOM data (integer data is exact in every reduction order and cannot see a change of
   kernel) and asserts bitwise equality of those rows in every output: f32, f16, e4m3 bytes and per-image statistics blocks.
B. Pitches and sentinels.  Every operand honours its row pitch (lda > K, ldr / ldo* / ld_row_add / ldx > N) and nothing is written
   outside [M) x [N): outputs are views into taller, wider buffers filled with NaN (f32 / f16) or 0x7F (e4m3), checked untouched.
   Integer data, exact against an fp64 reference.
C. col_scale is a mode-0 feature: a convolution with col_scale_n > 0 is refused (the window kernel never applied it).

Each case id names the kernel instantiation its shape steers to (csrc/gemm_plan.h: plan(), win_candidates(), the rows of
SEVA_GEMM_KERNELS / SEVA_WIN_KERNELS); tests/test_gemm_plan_cpu.py asserts that the planner says the same, and a kernel trace of this
file (rocprofv3 --kernel-trace --stats) lists them.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import rel_l2

U8 = torch.uint8
F16 = torch.float16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _ints(shape, lo, hi, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float().to(dev)


def _randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev) * scale


def _f8(x):
    from seva import ops
    return ops.to_fp8(x)


# ------------------------------------------------------------------------------------------------------------------------------
# A. batch invariance (random data, bitwise)
# ------------------------------------------------------------------------------------------------------------------------------
# Pinned elsewhere, not repeated here: the GEGLU f16 tile heights 64 / 128 / 160 (test_ops_gpu.py::test_geglu_tile_heights_bitwise_equal),
# the 160 x 160 fp32-output tiles against 128 / 64 rows (test_ops_gpu.py::test_tile_160x160_bitwise_equal), the window families among
# themselves (test_ops_gpu.py::test_conv3x3_window_kernel).

GEMM_A = [  # id (the instantiations the two launches take), M small, M large, N, K, kind
    # f16-only, K <= 320: 41 x 6 tiles of 128 rows < 320 -> 64-row ASYNC tiles; 81 x 6 -> 128-row A-in-registers tiles (the QKV
    # projection of one 72 x 72 frame vs two), with the q third scaled as the engine does
    ("f16only_async64_vs_astat128", 5184, 10368, 960, 320, "f16only"),
    # fp32 output: 64 x 160 (8 x 20 tiles) -> 128 x 160 (16 x 20, M < 2048) -> 160 x 160 (M >= 2048), with bias + row_add + residual
    ("f32_64x160_vs_128x160", 1000, 2047, 3200, 192, "f32"),
    ("f32_128x160_vs_160x160", 2047, 2600, 3200, 192, "f32"),
    ("f32_64x128_vs_128x128", 1000, 2047, 3204, 128, "f32"),
    # the narrow 128 x 32 kernel (N <= 32): the UNet head's 4 channels
    ("narrow_128x32", 1000, 5000, 4, 320, "f32"),
    # GEGLU f16-only, K <= 320: 64-row tiles (19 x 16 tiles) -> 128-row A-in-registers tiles
    ("geglu_f16only_64_vs_astat128", 2432, 5000, 2560, 320, "geglu16"),
    # e4m3: half_m8 64 x 160 -> 128 x 128 (plain), 64 x 128 -> 128 x 128 (GEGLU with the e4m3 out_f8 epilogue)
    ("fp8_64x160_vs_128x128", 4992, 6000, 1280, 640, "fp8"),
    ("fp8_geglu_outf8_64_vs_128", 2432, 5000, 2560, 640, "fp8geglu"),
]


@pytest.mark.parametrize("cid,m_small,m_large,N,K,kind", GEMM_A, ids=[c[0] for c in GEMM_A])
def test_gemm_rows_do_not_depend_on_m(dev, cid, m_small, m_large, N, K, kind, knobs):
    from seva import ops
    from seva._engine import interleave_geglu
    knobs(gemm_bm=-1, gemm_bn=-1, gemm_astat=-1, gemm_chunks=-1)
    fp8 = kind.startswith("fp8")
    geglu = kind in ("geglu16", "fp8geglu")
    nout = N // 2 if geglu else N
    a32 = _randn((m_large, K), dev, 1)
    w32 = _randn((N, K), dev, 2, K ** -0.5)
    bias = _randn((N,), dev, 3, 0.3)
    rpg = 81  # row_add groups that straddle both launches' tile boundaries
    radd = _randn(((m_large + rpg - 1) // rpg, N), dev, 4, 0.3)
    res = _randn((m_large, N), dev, 5)
    if geglu:
        w32, bias = interleave_geglu(w32, bias)
    if fp8:
        a = _f8(a32 * 8)
        w, w_exp = ops.quantize_weight_fp8(w32)
    else:
        a, w, w_exp = a32.half(), w32.half(), None

    def run(M):
        outs = {}
        kw = dict(bias=bias, w_exp=w_exp)
        if kind == "f16only":
            outs["f16"] = torch.full((M, nout), float("nan"), device=dev, dtype=F16)
            kw.update(out_f16=outs["f16"], col_scale=0.125 * 1.4426950408889634, col_scale_n=N // 3)
        elif kind == "geglu16":
            outs["f16"] = torch.full((M, nout), float("nan"), device=dev, dtype=F16)
            kw.update(out_f16=outs["f16"], geglu=True)
        elif kind == "fp8geglu":
            outs["f8"] = torch.full((M, nout), 0x7F, device=dev, dtype=U8)
            kw.update(out_f8=outs["f8"], geglu=True)
        else:
            outs["f32"] = torch.full((M, nout), float("nan"), device=dev)
            kw.update(out_f32=outs["f32"], residual=res[:M], row_add=radd, rows_per_group=rpg)
            if kind == "fp8":
                outs["f16"] = torch.full((M, nout), float("nan"), device=dev, dtype=F16)
                kw.update(out_f16=outs["f16"])
        ops.gemm(a[:M], w, **kw)
        return outs

    small, large = run(m_small), run(m_large)
    torch.cuda.synchronize()
    for k in small:
        s, l = small[k], large[k][:m_small]
        if k != "f8":
            assert torch.isfinite(s.float()).all(), k
        assert torch.equal(s, l), f"{cid} {k}: rows 0..{m_small} differ between M={m_small} and M={m_large}"


def _conv_case(dev, n, ih, iw, cin, cout, *, seed, fp8=False, up=False):
    """random NHWC input (f16 or e4m3 bytes) and packed weights"""
    from seva import ops
    from seva._engine import pack_conv3x3
    x = _randn((n, ih, iw, cin), dev, seed)
    wc = _randn((cout, cin, 3, 3), dev, seed + 1, (9 * cin) ** -0.5)
    wp = pack_conv3x3(wc).float()
    if fp8:
        w8, w_exp = ops.quantize_weight_fp8(wp)
        return _f8(x * 8), w8, w_exp
    return x.half(), wp.half(), None


CONV_A = [  # id, n values, ih, iw, cin, cout, stride, up, stats, fp8, split-K workspace, pad_br_only
    # GroupNorm statistics at hw % 64 != 0 (60 x 60, 52 x 52): refused by the window kernel at EVERY batch size (it used to run at n = 1
    # only, the per-tap gather at n >= 2: a different reduction order)
    ("stats_60x60_hw_not_64", (1, 2, 3), 60, 60, 320, 320, 1, False, True, False, False, False),
    ("stats_52x52_hw_not_64", (1, 2, 3), 52, 52, 320, 320, 1, False, True, False, False, False),
    # the 160-column family, statistics (4-wave 128 x 160 / 8-wave 256 x 160 per the launch's quantisation)
    ("win160_stats_16x16", (1, 9), 16, 16, 320, 640, 1, False, True, False, False, False),
    # fused nearest-2x upsample, 160 columns
    ("win160_upsample", (1, 5), 18, 18, 320, 320, 1, True, False, False, False, False),
    # narrow 32-column window (N = 4, the UNet head)
    ("win_narrow_n4", (1, 3), 72, 72, 320, 4, 1, False, False, False, False, False),
    # 128-column family: linear tiles (72 px rows) and 2-D tiles (144 px rows), plain and upsampled
    ("win128_linear", (1, 2), 72, 72, 128, 128, 1, False, True, False, False, False),
    ("win128_2d", (1, 2), 144, 144, 64, 128, 1, False, True, False, False, False),
    ("win128_2d_upsample", (1, 2), 72, 72, 64, 128, 1, True, False, False, False, False),
    # stride 2: per-tap gather, 64 x 160 tiles at n = 1 (M = 324) -> 160 x 160 at n = 42; pad_br_only (VAE Downsample2D)
    ("pertap_stride2_64_vs_160rows", (1, 42), 36, 36, 320, 640, 2, False, False, False, False, False),
    ("pertap_stride2_pad_br_only", (1, 40), 16, 16, 128, 128, 2, False, False, False, False, True),
    # split-K = 2 on 9 x 9 images (per-sample rule) with its workspace
    ("splitk_9x9", (1, 42), 9, 9, 1280, 1280, 1, False, False, False, True, False),
    # e4m3 window conv (128-column family, FP8 instantiations), with and without statistics
    ("fp8_win_36x36", (1, 6), 36, 36, 640, 640, 1, False, False, True, False, False),
    ("fp8_win_stats_16x16", (1, 5), 16, 16, 256, 384, 1, False, True, True, False, False),
    # the UNet's lower levels at the non-square latents 72x96 / 72x128: producer statistics at C = 640 (1728 pixels) and C = 1280
    # (576 pixels); 9 x 16 at C = 1280 with the engine's workspace: hw = 144 > 128, so NOT split (window kernel) at every batch size
    ("win160_stats_36x48_c640", (1, 3, 16), 36, 48, 640, 640, 1, False, True, False, False, False),
    ("win160_stats_18x32_c1280", (1, 3, 42), 18, 32, 1280, 1280, 1, False, True, False, False, False),
    ("win160_9x16_c1280_hw144_unsplit", (1, 3, 42), 9, 16, 1280, 1280, 1, False, False, False, True, False),
]


def _conv_run(x, w, w_exp, *, stride, up, pad_br, bias, emb, res, stats, ws, dev, n_out_rows, cout, f16=False):
    from seva import ops
    n = x.shape[0]
    hw = n_out_rows // n
    out = torch.full((n, hw, cout), float("nan"), device=dev)
    o16 = torch.full((n, hw, cout), float("nan"), device=dev, dtype=F16) if f16 else None
    st = torch.full(ops.channel_stats_shape(n_out_rows, cout), float("nan"), device=dev) if stats else None
    ops.conv3x3(x, w, w_exp=w_exp, stride=stride, upsample=up, pad_br_only=pad_br, bias=bias, row_add=emb, rows_per_group=hw,
                residual=res, out_f32=out, out_f16=o16, ch_stats=st, splitk_ws=ws)
    return (out, st, o16) if f16 else (out, st)


@pytest.mark.parametrize("cid,ns,ih,iw,cin,cout,stride,up,stats,fp8,sk,pad_br", CONV_A, ids=[c[0] for c in CONV_A])
def test_conv_frames_do_not_depend_on_batch(dev, cid, ns, ih, iw, cin, cout, stride, up, stats, fp8, sk, pad_br, knobs):
    """Frame 0 and frame n - 1 of every batch size in `ns` are bitwise the frame computed alone: f32 output (bias + per-frame row_add +
    residual) and, with statistics, the frame's own 64-row blocks (hw % 64 == 0: whole blocks; else the blocks inside frame 0)."""
    from seva import ops
    knobs(conv_win=-1, gemm_bm=-1, gemm_bn=-1)
    nmax = max(ns)
    x, w, w_exp = _conv_case(dev, nmax, ih, iw, cin, cout, seed=10, fp8=fp8)
    sc = 2 if up else 1
    ps = 1 if pad_br else 2
    oh, ow = (sc * ih + ps - 3) // stride + 1, (sc * iw + ps - 3) // stride + 1
    hw = oh * ow
    bias = _randn((cout,), dev, 20, 0.3)
    emb = _randn((nmax, cout), dev, 21, 0.3)
    res = _randn((nmax, hw, cout), dev, 22)
    ws = ops.splitk_workspace(nmax * hw, cout, dev) if sk else None
    kw = dict(stride=stride, up=up, pad_br=pad_br, bias=bias, stats=stats, ws=ws, dev=dev, cout=cout)

    def frame(i):
        return _conv_run(x[i:i + 1], w, w_exp, emb=emb[i:i + 1], res=res[i:i + 1], n_out_rows=hw, **kw)

    blocks = hw // 64  # statistics blocks that lie inside one frame when the frame starts on a block
    alone = {}
    for n in ns:
        out, st = _conv_run(x[:n], w, w_exp, emb=emb[:n], res=res[:n], n_out_rows=n * hw, **kw)
        for i in sorted({0, n - 1}):
            if i not in alone:
                alone[i] = frame(i)
            o1, s1 = alone[i]
            assert torch.isfinite(o1).all()
            assert torch.equal(out[i], o1[0]), f"{cid}: frame {i} of a batch of {n} differs from the frame alone"
            if stats and (hw % 64 == 0 or i == 0):
                b0 = i * hw // 64
                assert torch.equal(st[b0:b0 + blocks], s1[:blocks]), f"{cid}: statistics of frame {i} (batch {n})"
        if ws is not None:
            ops.check_handoffs()


def test_conv_72x72_window_at_the_32bit_index_limit(dev, knobs):
    """72 x 72 x 320 -> 320 with statistics (the headline latent's ResBlock conv): the linear window tiles index a launch with 32-bit
    multiply-high divisions that are exact up to 191 images.  Batch 192 (T = 96 with CFG) must still give every frame the bits it has
    alone -- it used to fall back to the per-tap gather.  Every per-image operand (input, residual, row_add, f32 / f16 outputs,
    statistics) is checked on the frames after the 191st.  About 4 GB of device memory."""
    knobs(conv_win=-1, gemm_bm=-1, gemm_bn=-1)
    n, hw, cout = 192, 72 * 72, 320
    x, w, _ = _conv_case(dev, n, 72, 72, 320, cout, seed=30)
    bias = _randn((cout,), dev, 31, 0.3)
    emb = _randn((n, cout), dev, 32, 0.3)
    res = _randn((n, hw, cout), dev, 33)
    kw = dict(stride=1, up=False, pad_br=False, bias=bias, stats=True, ws=None, dev=dev, cout=cout, f16=True)
    alone = {i: _conv_run(x[i:i + 1], w, None, emb=emb[i:i + 1], res=res[i:i + 1], n_out_rows=hw, **kw) for i in (0, 190, 191)}
    for nb in (191, 192):
        out, st, o16 = _conv_run(x[:nb], w, None, emb=emb[:nb], res=res[:nb], n_out_rows=nb * hw, **kw)
        for i in (0, nb - 1):
            o1, s1, h1 = alone[i]
            assert torch.isfinite(o1).all()
            assert torch.equal(out[i], o1[0]), f"frame {i} of a batch of {nb} differs from the frame alone"
            assert torch.equal(o16[i], h1[0]), f"f16 output of frame {i} (batch {nb})"
            assert torch.equal(st[i * 81:(i + 1) * 81], s1), f"statistics of frame {i} (batch {nb})"
        del out, st, o16
    torch.cuda.empty_cache()


@pytest.mark.parametrize("groups", [False, True], ids=["n_lin3", "row_add_groups_n_lin2"])
def test_conv_ranges_of_whole_images(dev, groups, knobs):
    """1024 x 32 px x 64 -> 128 with statistics: hw = 2^15, so the multiply-high divisions of the linear window tiles are exact only while
    n * hw^2 < 2^32 -- three images -- and a batch of 7 is launched as ranges of 3 + 3 + 1 whole images (csrc/gemm_plan.h: n_lin,
    plan_tiling; csrc/conv_win.hip: launch_win).  With row_add groups of two images a range must end on a group boundary: 2 + 2 + 2 + 1.
    Every image of the batch (input, row_add group, f32 output, statistics blocks moved by whole images) has the bits it has alone."""
    from seva import ops
    knobs(conv_win=-1, gemm_bm=-1, gemm_bn=-1)
    n, ih, iw, cin, cout = 7, 1024, 32, 64, 128
    hw, per = ih * iw, ih * iw // 64
    x, w, _ = _conv_case(dev, n, ih, iw, cin, cout, seed=70)
    bias = _randn((cout,), dev, 71, 0.3)
    emb = _randn(((n + 1) // 2, cout), dev, 72, 0.3)

    def run(xs, radd):
        k = xs.shape[0]
        out = torch.full((k, hw, cout), float("nan"), device=dev)
        st = torch.full(ops.channel_stats_shape(k * hw, cout), float("nan"), device=dev)
        ops.conv3x3(xs, w, bias=bias, row_add=radd, rows_per_group=2 * hw if groups else 0, out_f32=out, ch_stats=st)
        return out, st

    out, st = run(x, emb if groups else None)
    for i in range(n):
        o1, s1 = run(x[i:i + 1], emb[i // 2:i // 2 + 1] if groups else None)
        assert torch.isfinite(o1).all()
        assert torch.equal(out[i], o1[0]), f"image {i} of the batch differs from the image alone"
        assert torch.equal(st[i * per:(i + 1) * per], s1), f"statistics of image {i}"


# ------------------------------------------------------------------------------------------------------------------------------
# B. pitches and sentinels (integer data, exact against fp64)
# ------------------------------------------------------------------------------------------------------------------------------

def _pitched(M, N, dtype, dev):
    """(buffer, [M, N] view): the view starts one row down in a buffer two rows taller and 16-32 columns wider (row pitch a multiple of
    16 elements), filled with a sentinel: NaN, or 0x7F for e4m3 bytes"""
    ld = (N // 16 + 2) * 16
    fill = 0x7F if dtype == U8 else float("nan")
    buf = torch.full((M + 2, ld), fill, dtype=dtype, device=dev)
    return buf, buf[1:M + 1, :N]


def _untouched(buf, M, N):
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[1:M + 1, :N] = False
    rest = buf[outside]
    return bool((rest == 0x7F).all()) if buf.dtype == U8 else bool(torch.isnan(rest).all())


def _col_slice(t, off=64):
    """t as a column slice of a wider buffer (row pitch > width, 16-byte aligned start)"""
    buf = torch.zeros((t.shape[0], t.shape[1] + 2 * off), dtype=t.dtype, device=t.device)
    buf[:, off:off + t.shape[1]] = t
    return buf[:, off:off + t.shape[1]]


def _outputs(M, N, spec, dev):
    outs = {}
    if "f32" in spec:
        outs["f32"] = _pitched(M, N, torch.float32, dev)
    if "f16" in spec:
        outs["f16"] = _pitched(M, N, F16, dev)
    if "f8" in spec:
        outs["f8"] = _pitched(M, N, U8, dev)
    return outs


def _check_outputs(outs, ref, M, N, cid):
    """ref: exact fp64 values [M, N]"""
    for k, (buf, view) in outs.items():
        assert _untouched(buf, M, N), f"{cid}: {k} output written outside [M) x [N)"
        if k == "f32":
            assert torch.equal(view.double(), ref), f"{cid}: f32 max diff {(view.double() - ref).abs().max()}"
        elif k == "f16":
            assert torch.equal(view, ref.float().half()), f"{cid}: f16 output"
        else:
            assert torch.equal(view, _f8(ref.float())), f"{cid}: e4m3 output"


GEMM_B = [  # id (instantiation), M, N, K, outputs, epilogue extras
    ("f16_64x160", 1000, 640, 320, "f32 f16", "res radd"),
    ("f16_64x128", 1000, 516, 192, "f32 f16", "res radd"),
    ("f16_128x160", 2047, 3200, 192, "f32", "res radd"),
    ("f16_128x128", 2047, 3204, 128, "f32", "res radd"),
    ("f16_160x160", 2600, 3200, 192, "f32", "res radd"),
    ("f16_narrow_128x32", 1000, 12, 320, "f32 f16", "res radd"),
    ("f16only_async_64x160", 1000, 960, 320, "f16", "colscale"),
    ("f16only_astat_128x160", 7000, 960, 320, "f16", "colscale"),
    ("f16only_async_128x160", 7000, 960, 640, "f16", ""),
    ("geglu_64x128", 500, 1280, 640, "f32 f16", "geglu"),
    ("geglu_160x128", 1500, 1280, 640, "f32 f16", "geglu"),
    ("geglu_128x128", 7000, 1280, 320, "f32 f16", "geglu"),
    ("geglu_astat_128x128", 7000, 1280, 320, "f16", "geglu"),
    ("fp8_64x160", 1000, 640, 640, "f32 f16", "fp8 res radd"),
    ("fp8_64x128", 1000, 528, 256, "f32", "fp8 res radd"),
    ("fp8_128x128", 6000, 1280, 256, "f32", "fp8 res radd"),
    ("fp8_geglu_outf8_64x128", 500, 1280, 640, "f8", "fp8 geglu"),
    ("fp8_geglu_outf8_128x128", 5000, 2560, 256, "f8", "fp8 geglu"),
]


def _geglu_weights(N, K, dev, seed):
    """integer GEGLU weights in the reference layout (value rows, then gate rows) whose gate lands in [10, 22], where gelu(g) == g in
    fp32 (erf saturates to 1): the GEGLU output is then an exact product of integers.  Value rows use the first 16 columns only."""
    nh = N // 2
    wv = torch.zeros((nh, K), device=dev)
    wv[:, :16] = _ints((nh, 16), -2, 2, dev, seed)
    wg = torch.zeros((nh, K), device=dev)
    wg[:, :2] = _ints((nh, 2), -1, 1, dev, seed + 1)
    b = torch.cat([_ints((nh,), -3, 3, dev, seed + 2), _ints((nh,), 14, 18, dev, seed + 3)])
    return torch.cat([wv, wg]), b


@pytest.mark.parametrize("cid,M,N,K,spec,extra", GEMM_B, ids=[c[0] for c in GEMM_B])
def test_gemm_pitches_and_sentinels(dev, cid, M, N, K, spec, extra, knobs):
    from seva import ops
    from seva._engine import interleave_geglu
    knobs(gemm_bm=-1, gemm_bn=-1, gemm_astat=-1, gemm_chunks=-1)
    fp8, geglu = "fp8" in extra, "geglu" in extra
    a = _ints((M, K), -2, 2, dev, 1)
    if geglu:
        w, bias = _geglu_weights(N, K, dev, 2)
        wk, bk = interleave_geglu(w, bias)
    else:
        w, bias = _ints((N, K), -3, 3, dev, 2), _ints((N,), -5, 5, dev, 3)
        wk, bk = w, bias
    wref = w.double()
    if fp8:
        g = torch.Generator().manual_seed(4)
        e = torch.randint(-2, 1, (N,), generator=g).to(dev)
        w_exp_k = ((interleave_geglu(w, e.float())[1] if geglu else e.float()) + 127).to(U8)  # scale bytes follow the row order
        wref = (w * torch.exp2(e.float())[:, None]).double()
        a_op, w_op = _col_slice(_f8(a)), _f8(wk)
    else:
        w_exp_k = None
        a_op, w_op = _col_slice(a.half()), wk.half()
    assert a_op.stride(0) > K
    y = a.double() @ wref.T + bias.double()
    nout = N // 2 if geglu else N
    kw = dict(bias=bk, w_exp=w_exp_k)
    if geglu:
        assert float(y[:, nout:].min()) >= 10.0
        ref = y[:, :nout] * F.gelu(y[:, nout:])
        kw["geglu"] = True
    else:
        ref = y
    if "colscale" in extra:
        ns = N // 3 // 4 * 4
        ref[:, :ns] *= 0.5
        kw.update(col_scale=0.5, col_scale_n=ns)
    if "res" in extra:
        res = _ints((M, N), -9, 9, dev, 5)
        kw["residual"] = _col_slice(res, 16)
        ref = ref + res.double()
    if "radd" in extra:
        rpg = 7  # does not divide M
        radd = _ints(((M + rpg - 1) // rpg, N), -3, 3, dev, 6)
        ra = _col_slice(radd, 16)
        kw.update(row_add=ra, rows_per_group=rpg, ld_row_add=ra.stride(0))
        ref = ref + radd.double().repeat_interleave(rpg, 0)[:M]
    outs = _outputs(M, nout, spec, dev)
    kw.update({f"out_{k}": v[1] for k, v in outs.items()})
    ops.gemm(a_op, w_op, **kw)
    torch.cuda.synchronize()
    _check_outputs(outs, ref, M, nout, cid)


def _conv_ref(x, w, stride, up, pad_br):
    """fp64 (CPU) reference of the 3x3 conv; x: [n, cin, ih, iw], w: [cout, cin, 3, 3] -> [n, oh * ow, cout]"""
    x, w = x.double().cpu(), w.double().cpu()
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=stride) if pad_br else F.conv2d(x, w, stride=stride, padding=1)
    n, cout = y.shape[:2]
    return y.permute(0, 2, 3, 1).reshape(n, -1, cout)


CONV_B = [  # id (instantiation), n, ih, iw, cin, cout, stride, up, stats, kind: win (default dispatch) / pertap (conv_win=0) / splitk / a2 / fp8
    ("win160_linear_batch_tiles_stats", 3, 16, 16, 128, 320, 1, False, True, "win"),
    ("win160_linear_per_image_tiles_stats", 2, 72, 72, 64, 320, 1, False, True, "win"),
    ("win160_upsample", 2, 9, 9, 128, 320, 1, True, False, "win"),
    ("win128_linear", 2, 32, 48, 64, 128, 1, False, True, "win"),
    ("win128_2d_stats", 1, 144, 144, 64, 128, 1, False, True, "win"),
    ("win128_2d_upsample", 1, 72, 72, 64, 128, 1, True, False, "win"),
    ("win_narrow_linear", 2, 36, 36, 128, 4, 1, False, False, "win"),
    ("win_narrow_2d", 1, 144, 144, 64, 8, 1, False, False, "win"),
    ("pertap_stride1", 2, 16, 12, 128, 320, 1, False, True, "pertap"),
    ("pertap_stride2", 2, 16, 12, 128, 160, 2, False, False, "pertap"),
    ("pertap_stride2_pad_br_only", 2, 16, 12, 64, 96, 2, False, False, "padbr"),
    ("pertap_upsample", 2, 8, 6, 64, 128, 1, True, False, "pertap"),
    ("splitk_9x9", 5, 9, 9, 1280, 320, 1, False, False, "splitk"),
    ("a2_folded", 2, 16, 16, 128, 320, 1, False, True, "a2"),
    ("fp8_win_stats", 2, 16, 16, 256, 384, 1, False, True, "fp8"),
    ("fp8_pertap_stride2", 2, 16, 16, 256, 256, 2, False, False, "fp8"),
]


@pytest.mark.parametrize("cid,n,ih,iw,cin,cout,stride,up,stats,kind", CONV_B, ids=[c[0] for c in CONV_B])
def test_conv_pitches_and_sentinels(dev, cid, n, ih, iw, cin, cout, stride, up, stats, kind, knobs):
    from seva import ops
    from seva._engine import pack_conv3x3
    knobs(conv_win=0 if kind in ("pertap", "padbr") else -1, gemm_bm=-1, gemm_bn=-1)
    pad_br = kind == "padbr"
    x = _ints((n, cin, ih, iw), -3, 3, dev, 1)
    wc = _ints((cout, cin, 3, 3), -2, 2, dev, 2)
    ref = _conv_ref(x, wc, stride, up, pad_br)
    hw = ref.shape[1]
    M = n * hw
    ref = ref.reshape(M, cout)
    wp = pack_conv3x3(wc).float()
    kw = {}
    if kind == "a2":
        k2 = 192
        a2 = _ints((M, k2), -2, 2, dev, 3)
        w2 = _ints((cout, k2), -2, 2, dev, 4)
        kw["a2"] = _col_slice(a2.half())
        assert kw["a2"].stride(0) > k2
        wp = torch.cat([wp, w2], 1)
        ref = ref + (a2.double() @ w2.double().T).cpu()
    if kind == "fp8":
        g = torch.Generator().manual_seed(5)
        e = torch.randint(-2, 1, (cout,), generator=g).to(dev)
        ref = _conv_ref(x, wc * torch.exp2(e.float())[:, None, None, None], stride, up, pad_br).reshape(M, cout)
        xk, wk, kw["w_exp"] = _f8(x.permute(0, 2, 3, 1).contiguous()), _f8(wp), (e + 127).to(U8)
    else:
        xk, wk = x.permute(0, 2, 3, 1).contiguous().half(), wp.half()
    if kind == "splitk":
        kw["splitk_ws"] = ops.splitk_workspace(M, cout, dev)
    bias = _ints((cout,), -5, 5, dev, 6)
    res = _ints((M, cout), -9, 9, dev, 7)
    rpg = 7  # groups that straddle images and tiles and do not divide M
    radd = _ints(((M + rpg - 1) // rpg, cout), -3, 3, dev, 8)
    ra = _col_slice(radd, 16)
    ref = ref.to(dev) + bias.double() + res.double() + radd.double().repeat_interleave(rpg, 0)[:M]
    outs = _outputs(M, cout, "f32 f16" if kind != "a2" else "f32", dev)
    st_buf = None
    if stats:
        nb = ops.channel_stats_shape(M, cout)[0]
        st_buf = torch.full((nb + 3, 2, cout), float("nan"), device=dev)
        kw["ch_stats"] = st_buf[:nb]
    ops.conv3x3(xk, wk, stride=stride, upsample=up, pad_br_only=pad_br, bias=bias, row_add=ra, rows_per_group=rpg,
                ld_row_add=ra.stride(0), residual=_col_slice(res, 16), out_f32=outs["f32"][1],
                out_f16=outs["f16"][1] if "f16" in outs else None, **kw)
    torch.cuda.synchronize()
    _check_outputs(outs, ref, M, cout, cid)
    if stats:
        nb = ops.channel_stats_shape(M, cout)[0]
        assert bool(torch.isnan(st_buf[nb:]).all()), f"{cid}: statistics written past their blocks"
        st = st_buf[:nb].double()
        per = hw // 64  # blocks of one image (any partition of its pixels: 2-D tiles number them inside the image)
        assert torch.equal(st[:, 0].view(n, per, cout).sum(1), ref.view(n, hw, cout).sum(1)), f"{cid}: block sums"
        assert torch.allclose(st[:, 1].view(n, per, cout).sum(1), (ref.view(n, hw, cout) ** 2).sum(1), rtol=1e-6, atol=0)
    if kind == "splitk":
        ops.check_handoffs()


def _ff_weights(C, dev):
    """integer feed-forward weights whose hidden activations are exact in f16 (gate in [10, 22]: gelu(g) == g in fp32)"""
    from seva._engine import interleave_geglu
    w1, b1 = _geglu_weights(8 * C, C, dev, 40)
    w2 = _ints((C, 4 * C), -1, 1, dev, 43)
    b2 = _ints((C,), -5, 5, dev, 44)
    w1i, b1i = interleave_geglu(w1, b1)
    return w1, b1, w1i.half(), b1i, w2, b2


@pytest.mark.parametrize("M,C", [(1000, 320), (77, 64), (515, 256)], ids=["ff_C320", "ff_C64_one_tile", "ff_C256"])
def test_ff_fused_pitches_and_sentinels(dev, M, C):
    """seva_ff_fused_f16 with lda > C, ldr / ldo32 / ldo16 > C: exact on integer data whose GEGLU hidden activations are exact in f16"""
    from seva import ops
    w1, b1, w1i, b1i, w2, b2 = _ff_weights(C, dev)
    a = _ints((M, C), -2, 2, dev, 45)
    res = _ints((M, C), -9, 9, dev, 46)
    y = a.double() @ w1.double().T + b1.double()
    assert float(y[:, 4 * C:].min()) >= 10.0
    hid = y[:, :4 * C] * F.gelu(y[:, 4 * C:])
    assert torch.equal(hid.float().half().double(), hid)  # the kernel's f16 rounding of the hidden tensor is exact here
    ref = hid @ w2.double().T + b2.double() + res.double()
    outs = _outputs(M, C, "f32 f16", dev)
    ops.ff_fused(_col_slice(a.half()), w1i, b1i, w2.half(), b2, residual=_col_slice(res, 16), out_f32=outs["f32"][1],
                 out_f16=outs["f16"][1])
    torch.cuda.synchronize()
    _check_outputs(outs, ref, M, C, f"ff_fused C={C}")


@pytest.mark.parametrize("M,C", [(1000, 320), (300, 128)], ids=["ff_ln_C320", "ff_ln_C128"])
def test_ff_fused_layernorm_prologue_pitches(dev, M, C):
    """The LayerNorm prologue variant reads ln_x through ldx > C (fp32 rows of a wider buffer).  Not exact (the normalised row is
    rounded to f16 in registers): against an fp64 reference within a bound, and nothing written outside the output views."""
    from seva import ops
    from seva._engine import interleave_geglu
    g = torch.Generator().manual_seed(50)
    x = (torch.randn(M, C, generator=g) * 2 + 0.3).to(dev)
    gm, bt = (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    w1 = (torch.randn(8 * C, C, generator=g) * C ** -0.5).half().to(dev)
    b1 = (0.3 * torch.randn(8 * C, generator=g)).to(dev)
    w2 = (torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5).half().to(dev)
    b2 = (0.3 * torch.randn(C, generator=g)).to(dev)
    res = torch.randn(M, C, generator=g).to(dev)
    w1i, b1i = interleave_geglu(w1, b1)
    xs = _col_slice(x, 32)
    assert xs.stride(0) > C
    outs = _outputs(M, C, "f32 f16", dev)
    ops.ff_fused(None, w1i, b1i, w2, b2, residual=_col_slice(res, 16), out_f32=outs["f32"][1], out_f16=outs["f16"][1],
                 ln_x=xs, ln_gamma=gm, ln_beta=bt)
    torch.cuda.synchronize()
    xd = x.double()
    ln = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5) * gm.double() + bt.double()
    y = ln @ w1.double().T + b1.double()
    ref = (y[:, :4 * C] * F.gelu(y[:, 4 * C:])) @ w2.double().T + b2.double() + res.double()
    for k, (buf, view) in outs.items():
        assert _untouched(buf, M, C), f"{k} output written outside [M) x [C)"
        assert torch.isfinite(view).all()
        err = rel_l2(view, ref)
        assert err < 2e-3, (k, err)  # f16 roundings of the normalised row and of the hidden tensor (measured ~5e-4)


# ------------------------------------------------------------------------------------------------------------------------------
# C. col_scale is mode 0 only
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
def test_conv_col_scale_is_refused(dev, stride):
    """seva_gemm_desc.col_scale in conv mode used to be applied by the per-tap kernel and ignored by the window kernel (a stride-1
    conv returned unscaled features, a stride-2 one scaled features).  No caller uses it: it is an error for every conv."""
    from seva import _native as nv
    from seva._engine import pack_conv3x3
    n, ih, iw, cin, cout = 2, 16, 16, 64, 320
    x = _ints((n, ih, iw, cin), -2, 2, dev, 60).half()
    w = pack_conv3x3(_ints((cout, cin, 3, 3), -1, 1, dev, 61)).half()
    oh, ow = (ih - 1) // stride + 1, (iw - 1) // stride + 1
    out = torch.full((n * oh * ow, cout), float("nan"), device=dev)
    d = nv.GemmDesc()
    d.a, d.w, d.out_f32 = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.M, d.N, d.K = n * oh * ow, cout, 9 * cin
    d.lda, d.ldo32 = cin, cout
    d.mode, d.epilogue = 1, 0
    d.n, d.ih, d.iw, d.cin, d.oh, d.ow, d.stride = n, ih, iw, cin, oh, ow, stride
    d.col_scale, d.col_scale_n = 0.5, 160
    with pytest.raises(nv.SevaNativeError, match="col_scale"):
        nv.check(nv.load().seva_gemm_f16(C.byref(d), nv.stream_ptr(dev)), "seva_gemm_f16(conv, col_scale)")
    d.col_scale_n = 0  # the same launch without it runs
    nv.check(nv.load().seva_gemm_f16(C.byref(d), nv.stream_ptr(dev)), "seva_gemm_f16(conv)")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
