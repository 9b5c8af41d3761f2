"""The GEMM / conv dispatch policy (csrc/gemm_plan.h) checked without a GPU.

csrc/gemm_plan_dump.cpp is the planner's consumer outside the library: plain C++17, built here with g++, it reads descriptor lines
and prints one plan line each.  Checked:

* closed dispatch: every plan of the sweep names a row of the instantiation tables (a launcher would otherwise report an internal error);
* documented dispatch: the case ids of tests/test_gemm_contract_gpu.py (GEMM_A, CONV_A) name the instantiations their launches take,
  and the boundaries the code comments state sit where they say;
* batch invariance of what changes bits: window kernel or gather, split-K or not, linear or 2-D window tiles and n_lin are the same for
  every batch size of a per-sample shape (tile height, 4 vs 8 waves and the A-in-registers variant may follow the batch: they are pinned
  bitwise equal on the device);
* every benchmark knob gives the plan its comment describes.
"""
import pytest

from conftest import PKG
from kernel_cases import CXX, build_plan_dump, line

pytestmark = pytest.mark.skipif(CXX is None, reason="no g++")

BATCHES = (1, 2, 3, 7, 42)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """plans(lines) -> list of dicts, one per descriptor line (kernel_cases.build_plan_dump)"""
    return build_plan_dump(tmp_path_factory.mktemp("gemm_plan"), PKG)


def gemm(kind, M, N, K, **kw):
    """the launches of test_gemm_contract_gpu.py::test_gemm_rows_do_not_depend_on_m"""
    d = dict(v="fp8" if kind.startswith("fp8") else "f16", mode=0, M=M, N=N, K=K, bias=1)
    if kind == "f16only":
        d.update(out_f16=1)
    elif kind == "geglu16":
        d.update(out_f16=1, epi=1)
    elif kind == "fp8geglu":
        d.update(out_f8=1, epi=1, w_exp=1)
    else:
        d.update(out_f32=1, residual=1, row_add=1, rpg=81)
        if kind == "fp8":
            d.update(out_f16=1, w_exp=1)
    d.update(kw)
    return line(**d)


def conv(n, ih, iw, cin, cout, *, stride=1, up=0, stats=False, fp8=False, sk=False, pad_br=False, row_add=True, residual=True, out_f8=False,
         **kw):
    """a 3x3 conv as ops.conv3x3 / conv3x3_up_phases (up = 2) / conv3x3_up_phases128 (up = 4) state it"""
    sc = 2 if up else 1
    ps = 1 if pad_br else 2
    oh, ow = (sc * ih + ps - 3) // stride + 1, (sc * iw + ps - 3) // stride + 1
    phases = up in (2, 4)
    d = dict(v="fp8" if fp8 else "f16", mode=1, M=n * oh * ow, N=cout, K=(4 if phases else 9) * cin, n=n, ih=ih, iw=iw, cin=cin, oh=oh, ow=ow,
             stride=stride, up=up, pad_br=int(pad_br), bias=1, out_f32=1, ch_stats=int(stats), w_exp=int(fp8), out_f8=int(out_f8))
    if not phases:
        d.update(row_add=int(row_add), rpg=oh * ow, residual=int(residual), splitk_ws=int(sk))
    d.update(kw)
    return line(**d)


# ------------------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------------------

def test_tables_have_unique_rows_and_names(dump):
    rows = dump.tables()
    for table, count, dbg in (("gemm", 46, 27), ("win", 35, 0)):  # the library's instantiations (gemm: + 27 ablation twins = 73 kernels)
        sel = [r for r in rows if r["table"] == table]
        assert len(sel) == count
        assert len({r["name"] for r in sel}) == count, f"{table}: a name is used twice"
        cfgs = {tuple(v for k, v in r.items() if k not in ("table", "row", "name", "has_dbgk")) for r in sel}
        assert len(cfgs) == count, f"{table}: an instantiation is listed twice"
        assert sum(int(r.get("has_dbgk", 0)) for r in sel) == dbg


# ------------------------------------------------------------------------------------------------------------------------------------
# documented dispatch: the case ids of the contract suite
# ------------------------------------------------------------------------------------------------------------------------------------

GEMM_A_PLANS = {  # case id of test_gemm_contract_gpu.GEMM_A -> (row of the small launch, row of the large launch)
    "f16only_async64_vs_astat128": ("gemm 64x160 f16-only", "gemm 128x160 f16-only A-in-regs"),
    "f32_64x160_vs_128x160": ("gemm 64x160 f32", "gemm 128x160 f32"),
    "f32_128x160_vs_160x160": ("gemm 128x160 f32", "gemm 160x160 f32"),
    "f32_64x128_vs_128x128": ("gemm 64x128 f32", "gemm 128x128 f32"),
    "narrow_128x32": ("gemm 128x32 f32 narrow", "gemm 128x32 f32 narrow"),
    "geglu_f16only_64_vs_astat128": ("geglu 64x128", "geglu 128x128 A-in-regs"),
    "fp8_64x160_vs_128x128": ("gemm 64x160 e4m3 f32", "gemm 128x128 e4m3 f32"),
    "fp8_geglu_outf8_64_vs_128": ("geglu 64x128 e4m3", "geglu 128x128 e4m3"),
}

W160S = {"win 4-wave 128x160 linear stats", "win 8-wave 256x160 linear stats"}  # the two bitwise-equal families: either, by quantisation
W160U = {"win 4-wave 128x160 linear upsample", "win 8-wave 256x160 linear upsample"}
CONV_A_PLANS = {  # case id of test_gemm_contract_gpu.CONV_A -> allowed rows per batch size of the case
    "stats_60x60_hw_not_64": [{"conv gather 128x160"}] * 3,
    "stats_52x52_hw_not_64": [{"conv gather 128x160"}] * 3,
    "win160_stats_16x16": [W160S] * 2,
    "win160_upsample": [W160U] * 2,
    "win_narrow_n4": [{"win 4-wave 160x32 linear narrow"}] * 2,
    "win128_linear": [{"win 4-wave 128x128 linear stats"}] * 2,
    "win128_2d": [{"win 4-wave 128x128 2-D stats"}] * 2,
    "win128_2d_upsample": [{"win 4-wave 128x128 2-D upsample"}] * 2,
    "pertap_stride2_64_vs_160rows": [{"conv gather 64x160"}, {"conv gather 160x160"}],
    # 8 x 8 outputs: M = 64 at n = 1 is not "> 64" -> 128 rows; 20 x 1 tiles at n = 40 -> 64 rows
    "pertap_stride2_pad_br_only": [{"conv gather 128x128"}, {"conv gather 64x128"}],
    "splitk_9x9": [{"conv gather 128x160 split-K"}] * 2,
    "fp8_win_36x36": [{"win e4m3 4-wave 128x128 linear stats"}] * 2,
    "fp8_win_stats_16x16": [{"win e4m3 4-wave 128x128 linear stats"}] * 2,
    # the UNet's /2, /4 and /8 levels at the non-square latents 72x96 and 72x128
    "win160_stats_36x48_c640": [W160S] * 3,
    "win160_stats_18x32_c1280": [W160S] * 3,
    "win160_9x16_c1280_hw144_unsplit": [{"win 4-wave 160x160 linear", "win 8-wave 256x160 linear stats"}] * 3,
}


def test_contract_suite_case_ids_name_their_instantiations(dump):
    import test_gemm_contract_gpu as contract
    assert {c[0] for c in contract.GEMM_A} == set(GEMM_A_PLANS) and {c[0] for c in contract.CONV_A} == set(CONV_A_PLANS)
    for cid, m_small, m_large, N, K, kind in contract.GEMM_A:
        got = tuple(p["name"] for p in dump([gemm(kind, m_small, N, K), gemm(kind, m_large, N, K)]))
        assert got == GEMM_A_PLANS[cid], cid
    for cid, ns, ih, iw, cin, cout, stride, up, stats, fp8, sk, pad_br in contract.CONV_A:
        plans = dump([conv(n, ih, iw, cin, cout, stride=stride, up=int(up), stats=stats, fp8=fp8, sk=sk, pad_br=pad_br) for n in ns])
        for n, p, allowed in zip(ns, plans, CONV_A_PLANS[cid]):
            assert p["name"] in allowed, (cid, n, p["name"])
            assert p["kernel"] == ("window" if p["name"].startswith("win") else "gemm")


def test_the_72x72_window_runs_in_ranges_of_191_images(dump):
    """test_gemm_contract_gpu.py::test_conv_72x72_window_at_the_32bit_index_limit: exact up to 191 images, 192 = 191 + 1"""
    p191, p192 = dump([conv(n, 72, 72, 320, 320, stats=True, out_f16=1) for n in (191, 192)])
    assert p191["name"] in W160S and p192["name"] in W160S
    assert (p191["n_lin"], p191["ranges"], p192["n_lin"], p192["ranges"]) == ("191", "1", "191", "2")
    assert p192["n_full"] == "1" and p192["tail"].split("/")[0] == "1"


def test_the_n_lin_case_of_the_contract_suite(dump):
    """test_gemm_contract_gpu.py::test_conv_ranges_of_whole_images: 1024 x 32 px, hw = 2^15: n * hw^2 < 2^32 -> 3 images per range, 2 where
    the row_add groups span two images; linear tiles (32 px rows fit the window)"""
    kw = dict(stats=True, residual=False)
    plain, grouped = dump([conv(7, 1024, 32, 64, 128, row_add=False, **kw), conv(7, 1024, 32, 64, 128, row_add=True, rpg=2 * 32768, **kw)])
    for p, n_lin, ranges in ((plain, 3, 3), (grouped, 2, 4)):
        assert p["name"] == "win 4-wave 128x128 linear stats" and p["linear"] == "1"
        assert (int(p["n_lin"]), int(p["ranges"])) == (n_lin, ranges)


# ------------------------------------------------------------------------------------------------------------------------------------
# the boundaries the comments state
# ------------------------------------------------------------------------------------------------------------------------------------

def _names(dump, lines):
    return [p["name"] for p in dump(lines)]


def test_boundaries(dump):
    f32 = lambda M, N, K=192, **kw: gemm("f32", M, N, K, **kw)
    f16 = lambda M, N, K=640, **kw: gemm("f16only", M, N, K, **kw)
    # 160 x 160 tiles from M = 2048
    assert _names(dump, [f32(2047, 3200), f32(2048, 3200)]) == ["gemm 128x160 f32", "gemm 160x160 f32"]
    # 64-row tiles while ceil(M / 128) * ceil(N / 160) < 320, and only for M > 64
    assert _names(dump, [f16(319 * 128, 160), f16(319 * 128 + 1, 160)]) == ["gemm 64x160 f16-only", "gemm 128x160 f16-only"]
    assert _names(dump, [f16(64, 160), f16(65, 160)]) == ["gemm 128x160 f16-only", "gemm 64x160 f16-only"]
    # split-K: at most 128 output pixels per sample, K / 64 >= 16 and even (cin 64: 9 K-tiles, 128: 18, 192: 27)
    sk = lambda ih, iw, cin: conv(5, ih, iw, cin, 320, sk=True)
    plans = dump([sk(8, 16, 1280), sk(3, 43, 1280), sk(9, 9, 64), sk(9, 9, 128), sk(9, 9, 192)])
    assert [p.get("splitk", "0") for p in plans] == ["1", "0", "0", "1", "0"]
    assert plans[0]["name"] == plans[3]["name"] == "conv gather 128x160 split-K" and plans[0]["grid"] == str(2 * 5 * 2)
    assert all(p["kernel"] == "window" for p in (plans[1], plans[2], plans[4]))  # not split: the window kernel takes them
    # the A-in-registers variant up to K = 320
    assert _names(dump, [f16(10368, 960, 320), f16(10368, 960, 384)]) == ["gemm 128x160 f16-only A-in-regs", "gemm 128x160 f16-only"]
    # width: N % 160 == 0 -> 160 columns, else 128; N <= 32 -> the narrow kernel
    assert _names(dump, [f32(2047, 3200), f32(2047, 3328), f32(2047, 32), f32(2047, 36)]) == [
        "gemm 128x160 f32", "gemm 128x128 f32", "gemm 128x32 f32 narrow", "gemm 64x128 f32"]
    c = lambda cout: conv(2, 36, 36, 320, cout)
    names = _names(dump, [c(320), c(384), c(4), c(36)])
    assert names[0] in {"win 4-wave 160x160 linear", "win 8-wave 256x160 linear stats"}
    assert names[1:] == ["win 4-wave 128x128 linear stats", "win 4-wave 160x32 linear narrow", "conv gather 64x128"]
    # the split-precision output: one tile shape per epilogue and width, whatever M
    so = lambda M, N, **kw: line(v="split_out", mode=0, M=M, N=N, K=320, out_f16=1, bias=1, **kw)
    assert _names(dump, [so(100, 320), so(50000, 320), so(100, 384), so(50000, 2560, epi=1)]) == [
        "gemm 128x160 split-out", "gemm 128x160 split-out", "gemm 128x128 split-out", "geglu 128x128 split-out"]


# ------------------------------------------------------------------------------------------------------------------------------------
# batch invariance of what changes bits, closed dispatch
# ------------------------------------------------------------------------------------------------------------------------------------

def _sweep():
    """(per-sample shape id, conv(n, ...) arguments)"""
    shapes = []
    add = lambda sid, *a, **kw: shapes.append((sid, a, kw))
    # the UNet's levels: 3x3 convs at stride 1, stride 2 and with the fused upsample; statistics, row_add, split-K workspace on and off
    for side in (72, 36, 18, 9):
        for c in (320, 640, 1280):
            for stride, up in ((1, 0), (2, 0), (1, 1)):
                for stats in (False, True):
                    for radd in (False, True):
                        for sk in (False, True):
                            add(f"unet{side}_c{c}_s{stride}_u{up}_st{stats:d}_ra{radd:d}_sk{sk:d}", side, side, c, c, stride=stride, up=up, stats=stats,
                                row_add=radd, sk=sk)
            if c >= 640:  # the fp8 precision mode's levels
                for stats in (False, True):
                    add(f"unet{side}_c{c}_fp8_st{stats:d}", side, side, c, c, stats=stats, fp8=True)
                    add(f"unet{side}_c{c}_fp8_s2_st{stats:d}", side, side, c, c, stride=2, stats=stats, fp8=True)
            for cout in (4, 8):  # the head
                add(f"unet{side}_c{c}_head{cout}", side, side, c, cout, row_add=False, residual=False)
            if side <= 36:  # the three Upsample convs as phase convs
                add(f"unet{side}_c{c}_phases", side, side, c, c, up=2)
    # the UNet's levels at the non-square latents 72x96 (768x576 px), 96x72 and 72x128 (1024x576 px): widths 12 ... 128; 1728, 2304 and 576
    # pixels take producer statistics at C = 640 / 1280, 108 pixels are split (hw <= 128), 144 are not
    for top_h, top_w in ((72, 96), (96, 72), (72, 128)):
        for lvl in range(4):
            ih, iw = top_h >> lvl, top_w >> lvl
            for c in (320, 640, 1280):
                for stride, up in ((1, 0), (2, 0), (1, 1)):
                    for stats in (False, True):
                        for sk in (False, True):
                            add(f"unet{ih}x{iw}_c{c}_s{stride}_u{up}_st{stats:d}_sk{sk:d}", ih, iw, c, c, stride=stride, up=up, stats=stats, sk=sk)
                add(f"unet{ih}x{iw}_c{c}_head4", ih, iw, c, 4, row_add=False, residual=False)
                if lvl:
                    add(f"unet{ih}x{iw}_c{c}_phases", ih, iw, c, c, up=2)
    # the widths of ADVICE.md finding 1, with statistics
    for w in range(51, 78):
        add(f"advice{w}", w, w, 320, 320, stats=True)
        add(f"advice{w}_c640", w, w, 320, 640, stats=True)
    # ragged images
    for ih, iw in ((8, 24), (16, 8)):
        for stats in (False, True):
            add(f"ragged{ih}x{iw}_st{stats:d}", ih, iw, 320, 320, stats=stats)
            add(f"ragged{ih}x{iw}_c128_st{stats:d}", ih, iw, 128, 128, stats=stats)
    # the VAE: 72 .. 576 px at 128 / 256 / 512 channels, f16 and e4m3, the e4m3 output, the upsample convs (fused and as phases)
    for side in (72, 144, 288, 576):
        for c in (128, 256, 512):
            for fp8 in (False, True):
                for stats in (False, True):
                    add(f"vae{side}_c{c}_f8{fp8:d}_st{stats:d}", side, side, c, c, stats=stats, fp8=fp8, row_add=False)
                    if side <= 288:
                        add(f"vae{side}_c{c}_f8{fp8:d}_st{stats:d}_up", side, side, c, c, up=1, stats=stats, fp8=fp8, row_add=False, residual=False)
                if fp8:
                    add(f"vae{side}_c{c}_outf8", side, side, c, c, fp8=True, out_f8=True, row_add=False)
            if side <= 288:
                for stats in (False, True):
                    add(f"vae{side}_c{c}_phases_st{stats:d}", side, side, c, c, up=4, stats=stats)
            add(f"vae{side}_c{c}_convout", side, side, c, 4, row_add=False, residual=False)
            # the fp8 encoder's stride-2 bottom / right-padded convs: the gather by default, the window family under conv_win 1 / 2
            for knob in (-1, 1, 2):
                for stats in (False, True):
                    add(f"vaeenc{side}_c{c}_win{knob}_st{stats:d}", side, side, c, c, stride=2, pad_br=True, fp8=True, stats=stats, row_add=False,
                        residual=False, conv_win=knob)
            add(f"vaeenc{side}_c{c}_f16", side, side, c, c, stride=2, pad_br=True, row_add=False, residual=False)
    return shapes


def test_batch_invariance_and_closed_dispatch(dump):
    shapes = _sweep()
    lines = [conv(n, *a, **kw) for _, a, kw in shapes for n in BATCHES]
    assert 2000 < len(lines) < 10000
    plans = dump(lines)
    n_window = n_ranges = 0
    for i, (sid, _, _) in enumerate(shapes):
        per_n = plans[i * len(BATCHES):(i + 1) * len(BATCHES)]
        sigs = set()
        for n, p in zip(BATCHES, per_n):
            # closed dispatch: the plan and every candidate tried name a table row
            assert p["kernel"] in ("gemm", "window", "error"), (sid, n, p)
            if p["kernel"] != "error":
                assert int(p["row"]) >= 0 and p["name"] != "NONE", (sid, n, p)
            assert "NONE" not in p["cands"].split(";"), (sid, n, p)
            if p["kernel"] == "window":
                sigs.add(("window", p["linear"], p["n_lin"]))
                n_window += 1
                n_ranges += int(p["ranges"]) > 1
                # the ranges cover the batch, none longer than n_lin
                full_n, tail_n = int(p["full"].split("/")[0]), int(p["tail"].split("/")[0])
                assert int(p["n_full"]) * full_n + tail_n == n, (sid, n, p)
                assert p["linear"] == "0" or max(full_n, tail_n) <= int(p["n_lin"]), (sid, n, p)
            elif p["kernel"] == "gemm":
                sigs.add(("gather", "split-K" if p["splitk"] == "1" else "unsplit"))
            else:
                sigs.add(("error", p["declined"]))
        assert len(sigs) == 1, f"{sid}: what changes bits depends on the batch: {sorted(sigs)}"
    assert n_window > 1000 and n_ranges > 0  # the sweep reaches the window kernel, and its ranges of whole images (576 px at n = 42)


# ------------------------------------------------------------------------------------------------------------------------------------
# knobs
# ------------------------------------------------------------------------------------------------------------------------------------

def test_knobs(dump):
    f32 = lambda M, N=3200, **kw: gemm("f32", M, N, 192, **kw)
    # gemm_bm forces the tile height
    assert _names(dump, [f32(10368, gemm_bm=64), f32(10368, gemm_bm=128), f32(1000, gemm_bm=160), f32(10368)]) == [
        "gemm 64x160 f32", "gemm 128x160 f32", "gemm 160x160 f32", "gemm 160x160 f32"]
    # gemm_bn forces the width (and with it 128-row tiles: 160 x 160 is a fixed shape)
    assert _names(dump, [f32(10368, gemm_bn=128), f32(10368, 3328, gemm_bn=160)]) == ["gemm 128x128 f32", "gemm 128x160 f32"]
    # gemm_astat = 0: no A-in-registers variant
    assert _names(dump, [gemm("f16only", 10368, 960, 320, gemm_astat=0), gemm("geglu16", 5000, 2560, 320, gemm_astat=0)]) == [
        "gemm 128x160 f16-only", "geglu 128x128"]
    # gemm_chunks = n: n sibling workgroups per M-tile (at most one per N-tile), and no fixed-shape kernel
    p3, p99, p0 = dump([f32(10368, gemm_chunks=3), f32(10368, gemm_chunks=99), f32(2047)])
    assert (p3["name"], p3["chunks"], p3["grid"]) == ("gemm 128x160 f32", "3", str(81 * 3))
    assert (p99["chunks"], p99["tiles_n"]) == ("20", "20")
    # the heuristic: 20 N-tiles -> 4 per workgroup = 5 chunks, raised to >= 1024 / 16 M-tiles = 64 workgroups per M-tile, at most one per N-tile
    assert (p0["tiles_m"], p0["tiles_n"], p0["chunks"], p0["grid"]) == ("16", "20", "20", "320")
    # gemm_dbg / gemm_stagger > 0: the ablation twin; >= 0: no window kernel, no split-K, no A-in-registers, no 160-row tiles
    for knob in ("gemm_dbg", "gemm_stagger"):
        for val in (0, 2):
            kw = {knob: val}
            plans = dump([f32(10368, **kw), gemm("f16only", 10368, 960, 320, **kw), gemm("geglu16", 5000, 2560, 640, **kw),
                          conv(42, 9, 9, 1280, 1280, sk=True, **kw), conv(42, 72, 72, 320, 320, **kw)])
            assert [p["name"] for p in plans] == ["gemm 128x160 f32", "gemm 128x160 f16-only", "geglu 128x128", "conv gather 64x160",
                                                  "conv gather 128x160"], kw
            assert all(p["dbgk"] == str(int(val > 0)) and p["splitk"] == "0" for p in plans), kw
            assert all(p["dbg" if knob == "gemm_dbg" else "stagger"] == str(val) for p in plans), kw
    # ... but the e4m3 kernels have no ablation twin: a stagger run leaves the e4m3 window kernel on, a dbg run turns it off
    st, db = dump([conv(2, 36, 36, 640, 640, fp8=True, gemm_stagger=2), conv(2, 36, 36, 640, 640, fp8=True, gemm_dbg=2)])
    assert (st["kernel"], db["name"], db["dbgk"]) == ("window", "conv gather 64x160 e4m3", "0")  # (N = 640: 160 columns on 64-row tiles)
    # conv_win: 0 = the gather everywhere (an error for what only the window kernel runs), 1 = 4 waves, 2 = 8 waves
    c = lambda **kw: conv(42, 72, 72, 320, 320, stats=True, **kw)
    assert _names(dump, [c(conv_win=0), c(conv_win=1), c(conv_win=2)]) == [
        "conv gather 128x160", "win 4-wave 128x160 linear stats", "win 8-wave 256x160 linear stats"]
    off = dump([conv(2, 36, 36, 320, 320, up=2, conv_win=0), conv(2, 72, 72, 128, 128, up=4, conv_win=0),
                conv(2, 36, 36, 640, 640, fp8=True, out_f8=True, conv_win=0), conv(2, 36, 36, 640, 640, fp8=True, conv_win=0)])
    assert [(p["kernel"], p.get("declined")) for p in off[:3]] == [("error", "phases"), ("error", "phases"), ("error", "fp8_window_only")]
    assert off[3]["name"] == "conv gather 64x160 e4m3"
    ph = lambda knob: conv(2, 72, 72, 128, 128, up=4, stats=True, conv_win=knob)
    assert _names(dump, [ph(-1), ph(1), ph(2), conv(42, 36, 36, 320, 320, up=2, conv_win=1), conv(42, 36, 36, 320, 320, up=2, conv_win=2)]) == [
        "win phases 4-wave 128x128 linear stats", "win phases 4-wave 128x128 linear stats", "win phases 8-wave 256x128 linear stats",
        "win phases 4-wave 160x160 linear", "win phases 8-wave 256x160 linear"]
    # the e4m3 stride-2 window family runs only when asked for, and then declining is an error
    enc = lambda knob, **kw: conv(7, 288, 288, 128, 128, stride=2, pad_br=True, fp8=True, row_add=False, residual=False, conv_win=knob, **kw)
    plans = dump([enc(-1), enc(1), enc(2), conv(7, 100, 100, 128, 128, stride=2, pad_br=True, fp8=True, stats=True, conv_win=1)])
    assert plans[0]["name"] == "conv gather 128x128 e4m3"
    assert plans[1]["name"] == plans[2]["name"] == "win e4m3 4-wave 128x128 2-D stride 2"
    assert (plans[3]["kernel"], plans[3]["declined"]) == ("error", "fp8_stride2")  # 50 x 50 outputs: hw % 64 != 0 with statistics
