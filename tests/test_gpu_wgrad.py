"""GPU (-m gpu): every weight-gradient kernel din_conv_wgrad can launch, and the conv_wgrad_reduce_kernel epilogue it ends in, against a
float64 reference on the bf16-rounded (fp32: exact) operands.

One row of WGRAD_CASES per kernel instantiation; the row's DIN_* options force it, and both the kernel din_conv_kernel_names(d, 2) reports
(the row's `kernel`: the exact instantiation, as rocprofv3 prints it) and the code of din_conv_kernel_tile(d, 2) are asserted before
anything runs.  Every row carries the edges where such kernels go wrong: M not a multiple of 32, cout not a multiple of
the filter tile, kh*kw*cin_pad not a multiple of the k tile, channel views (cioff / cooff != 0, ldi > cin, ldo > cout).  Each row runs in
three epilogue modes:
  plain        scale = w = wdot = None, accumulate 0; dw / dbias prefilled with NaN, the launch must overwrite them;
  production   scale, w, wdot, dbias, accumulate 2 (what nhwc.py's backbone passes): dw overwritten, dbias / wdot added into;
  accumulate   accumulate 1 with scale, w, wdot: dw += scale * dW, dbias / wdot overwritten;
each twice (state carried between launches: the atomic-epilogue memset, the pacing tags) on a workspace full of 0x7f bytes, with guard
bands around dw / dbias / wdot.  The bars: dW max-rel 1e-5 (fp32: 5e-5); dbias / wdot per channel |err| <= 1e-5 * sum |terms|.  Each row
also checks on the CPU that its bar bites: dropping the last 32-pixel stage of M moves the reference by >= 10x the bar."""
import ctypes as C

import pytest
import torch

from oracle import din_oracle as O
from tests.conftest import Measured
from tests.test_gpu_kernels import PIPE_CASES, env, rel  # noqa: F401  (env: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

BAR = {"bf16": 1e-5, "fp32": 5e-5}        # dW and <w, dW>: fp32 sums of exact products (fp32 operands: fp32 products)
BAR_BIAS = 1e-5                           # column sums of the gradient operand
POISON = 1000.0                           # channels outside a tensor view (a kernel that reads them into dW fails the bar)
GUARD = -1234.5                           # guard bands around the outputs
NG = 256                                  # guard floats on each side (1 KiB: keeps the 16-byte alignment of the outputs)


def _row(name, kernel, code, dtype, shape, ld, opts=None, **extra):
    """shape = (nb, cin, h, w, cout, k, s, p, d); ld = (ldi, cioff, ldo, cooff); kernel = the first line of din_conv_kernel_names(d, 2);
    code = din_conv_kernel_tile(d, 2) (bm, bn)"""
    return dict(name=name, kernel=kernel, code=code, dtype=dtype, shape=shape, ld=ld, opts=opts or {}, **extra)


def _pipe(name, bco, opts=None, **extra):
    nb, cin, h, w, cout, k, s, p = next(c[1:] for c in PIPE_CASES if c[0] == name)
    wide = (w + 2 * p[1] - k[1]) // s[1] + 1 >= 32            # WIDE: an output row holds a 32-pixel stage; WN = 8: the default sixteen-wave grid
    return _row(name, f"conv_wgrad_pipe_kernel<{bco}, 256, {'true' if wide else 'false'}, 8>", (bco, 2256), "bf16", (nb, cin, h, w, cout, k, s, p, 1),
                (cin + 16, 8, cout + 16, 8), dict({"DIN_WGRAD_PIPE": "1"}, **(opts or {})), **extra)


S1, S2, P0, P1 = (1, 1), (2, 2), (0, 0), (1, 1)
K3, K17, K71 = (3, 3), (1, 7), (7, 1)
RING0 = {"DIN_WGRAD_RING": "0"}
WGRAD_CASES = [
    # fp32 (conv_wgrad_f32_kernel): stride 2 + dilation 2, 7x1 without padding, two filter tiles
    _row("f32_3x3_s2_d2", "conv_wgrad_f32_kernel", (128, 128), "fp32", (2, 13, 27, 29, 40, K3, S2, (2, 2), 2), (20, 4, 48, 4)),
    _row("f32_7x1_p0", "conv_wgrad_f32_kernel", (128, 128), "fp32", (1, 20, 23, 19, 136, K71, S1, P0, 1), (28, 4, 148, 8)),
    # bf16, cin % 8 != 0 (conv_wgrad_bf16_tail_kernel): the RGB layer; 12 channels on 1x7 taps with cout % 8 != 0
    _row("tail_cin3", "conv_wgrad_bf16_tail_kernel", (128, 128), "bf16", (2, 3, 33, 41, 64, K3, S1, P1, 1), (16, 8, 80, 8)),
    _row("tail_cin12_1x7", "conv_wgrad_bf16_tail_kernel", (128, 128), "bf16", (1, 12, 21, 37, 42, K17, S1, (0, 3), 1), (24, 8, 64, 8)),
    # two-workgroups-per-CU kernel (conv_wgrad_bf16_kernel<BCO>), the ring kernels off
    _row("v3_64", "conv_wgrad_bf16_kernel<64>", (64, 128), "bf16", (2, 40, 19, 23, 56, K3, S1, P0, 1), (56, 8, 72, 8), RING0),
    _row("v3_96_1x7", "conv_wgrad_bf16_kernel<96>", (96, 128), "bf16", (2, 48, 17, 29, 88, K17, S1, (0, 3), 1), (64, 8, 104, 8), RING0),
    _row("v3_128", "conv_wgrad_bf16_kernel<128>", (128, 128), "bf16", (1, 32, 25, 27, 248, K3, S1, P1, 1), (48, 8, 264, 8), RING0),
    _row("v3_160_7x1", "conv_wgrad_bf16_kernel<160>", (160, 128), "bf16", (2, 24, 23, 13, 152, K71, S1, (3, 0), 1), (40, 8, 168, 8), RING0),
    # 8-wave ring, 128 k columns (conv_wgrad_ring_kernel<BCO, 128>): 64 / 96-row banks by default, 128 / 160 with DIN_WGRAD_RING=3
    _row("ring64_128", "conv_wgrad_ring_kernel<64, 128>", (64, 1128), "bf16", (2, 64, 21, 26, 48, K3, S1, P1, 1), (80, 8, 64, 8)),
    _row("ring96_128_5x5", "conv_wgrad_ring_kernel<96, 128>", (96, 1128), "bf16", (1, 40, 23, 31, 80, (5, 5), S1, (2, 2), 1), (56, 8, 96, 8)),
    _row("ring128_128_1x7", "conv_wgrad_ring_kernel<128, 128>", (128, 1128), "bf16", (2, 56, 19, 27, 104, K17, S1, (0, 3), 1), (72, 8, 120, 8),
         {"DIN_WGRAD_RING": "3"}),
    _row("ring160_128_p0", "conv_wgrad_ring_kernel<160, 128>", (160, 1128), "bf16", (2, 24, 29, 31, 152, K3, S1, P0, 1), (40, 8, 168, 8),
         {"DIN_WGRAD_RING": "3"}),
    # ring, 256 k columns (conv_wgrad_ring_kernel<BCO, 256>): the pipelined kernel off
    _row("ring128_256", "conv_wgrad_ring_kernel<128, 256>", (128, 1256), "bf16", (2, 48, 17, 23, 120, K3, S1, P1, 1), (64, 8, 136, 8),
         {"DIN_WGRAD_PIPE": "0", "DIN_WGRAD_RING": "2"}),
    _row("ring160_256_1x7", "conv_wgrad_ring_kernel<160, 256>", (160, 1256), "bf16", (2, 40, 15, 33, 152, K17, S1, (0, 3), 1),
         (56, 8, 168, 8), {"DIN_WGRAD_PIPE": "0", "DIN_WGRAD_RING": "2"}),
    _row("ring192_256_7x1", "conv_wgrad_ring_kernel<192, 256>", (192, 1256), "bf16", (1, 48, 29, 21, 184, K71, S1, (3, 0), 1),
         (64, 8, 200, 8), {"DIN_WGRAD_PIPE": "0", "DIN_WGRAD_RING": "2"}),
    # software-pipelined kernel (conv_wgrad_pipe.hip): 128 / 192 / 256-row banks, slice partials and the atomic epilogue, paced (2-3 k
    # tiles) and unpaced (more k tiles, DIN_WGRAD_PACE=0), and the single-slice 1x1 form that writes dW straight from its accumulators
    _pipe("pipe128_3x3", 128),
    _pipe("pipe128_3x3_narrow", 128),
    _pipe("pipe192_3x3_p0_tail", 192),
    _pipe("pipe192_7x1", 192),
    _pipe("pipe384_3x3_s2", 192, {"DIN_WGRAD_ATOMIC": "1"}),
    _pipe("pipe256_1x7", 256, {"DIN_WGRAD_PACE": "0"}),
    _pipe("pipe256_1x1_direct", 256, direct=True),
    # stem kernels (conv_wgrad_small_kernel, >= 256K output pixels): 32 -> <= 32, 32 -> <= 64 (three-slot ring, two-slot ring, four
    # waves), the image layer (prepared NHWC input and the raw uint8 frames)
    _row("small1", "conv_wgrad_small_kernel<4, 32, 1, false, 4, 8, 2>", (0, 32), "bf16", (2, 32, 363, 365, 24, K3, S1, P1, 1), (48, 8, 40, 8)),
    _row("small2_ring3", "conv_wgrad_small_kernel<4, 64, 1, false, 8, 6, 3>", (0, 64), "bf16", (2, 32, 365, 367, 56, K3, S1, P0, 1),
         (40, 8, 64, 8)),
    _row("small2_ring2", "conv_wgrad_small_kernel<4, 64, 1, false, 8, 8, 2>", (0, 64), "bf16", (2, 32, 363, 365, 40, K3, S1, P1, 1),
         (48, 8, 56, 8), {"DIN_WGRAD_SMALL_RING": "2"}),
    _row("small2_w4", "conv_wgrad_small_kernel<4, 64, 1, false, 4, 8, 2>", (0, 64), "bf16", (2, 32, 365, 367, 48, K3, S1, P0, 1), (40, 8, 64, 8),
         {"DIN_WGRAD_SMALL_WAVES": "4"}),
    _row("small3_image", "conv_wgrad_small_kernel<1, 32, 2, false, 4, 8, 2>", (0, 32), "bf16", (1, 5, 1031, 1029, 24, K3, S2, P1, 1), (16, 8, 40, 8)),
    _row("small3_image_u8", "conv_wgrad_small_kernel<1, 32, 2, true, 4, 8, 2>", (0, 32), "bf16", (1, 3, 1031, 1029, 24, K3, S2, P0, 1),
         (8, 0, 40, 8), u8=True),
    # stationary halo kernel (conv_wgrad_halo_kernel, the three shapes of wgrad_halo_shape), forced on small maps
    _row("halo_5x5_48_64", "conv_wgrad_halo_kernel<6, 32, 5, 5, 8>", (3, 32), "bf16", (2, 48, 37, 45, 64, (5, 5), S1, (2, 2), 1),
         (64, 8, 80, 8), {"DIN_WGRAD_HALO": "2"}),
    _row("halo_3x3_64_96", "conv_wgrad_halo_kernel<8, 48, 3, 3, 8>", (3, 48), "bf16", (2, 64, 35, 47, 96, K3, S1, P1, 1), (80, 8, 112, 8),
         {"DIN_WGRAD_HALO": "2"}),
    _row("halo_3x3_96_96_p0", "conv_wgrad_halo_kernel<12, 48, 3, 3, 4>", (3, 48), "bf16", (2, 96, 37, 41, 96, K3, S1, P0, 1),
         (112, 8, 112, 8), {"DIN_WGRAD_HALO": "2"}),
    # the three slice-group paths of conv_wgrad_reduce_kernel (slices < 8: one group, 8..63: four, >= 64: sixteen)
    _row("reduce_nsg1", "conv_wgrad_bf16_kernel<128>", (128, 128), "bf16", (4, 64, 31, 37, 120, K3, S1, P1, 1), (80, 8, 136, 8),
         dict(RING0, DIN_WGRAD_BLOCKS="20"), slices=(1, 7)),
    _row("reduce_nsg4", "conv_wgrad_bf16_kernel<128>", (128, 128), "bf16", (4, 64, 31, 37, 120, K3, S1, P1, 1), (80, 8, 136, 8),
         dict(RING0, DIN_WGRAD_BLOCKS="100"), slices=(8, 63)),
    _row("reduce_nsg16", "conv_wgrad_bf16_kernel<128>", (128, 128), "bf16", (4, 64, 31, 37, 120, K3, S1, P1, 1), (80, 8, 136, 8),
         dict(RING0, DIN_WGRAD_BLOCKS="2000"), slices=(64, 1 << 20)),
]
MODES = ("plain", "production", "accumulate")


def _pad(n, m):
    return (n + m - 1) // m * m


def _geometry(row):
    nb, cin, h, w, cout, k, s, p, dil = row["shape"]
    oh = (h + 2 * p[0] - dil * (k[0] - 1) - 1) // s[0] + 1
    ow = (w + 2 * p[1] - dil * (k[1] - 1) - 1) // s[1] + 1
    return nb, cin, h, w, cout, k, s, p, dil, oh, ow


def wgrad_reference(x, g, k, s, p, dil, oh, ow):
    """float64 dW_raw [cout][cin][kh][kw] = sum over pixels of g (x) the tap-shifted input, as one GEMM per tap; and the same sum over
    the last 32-pixel stage of M only (what a kernel that lost that stage would miss).  x: [nb][h][w][cin], g: [M][cout], float64."""
    nb, h, w, cin = x.shape
    M, cout = g.shape
    xp = torch.nn.functional.pad(x, (0, 0, p[1], p[1], p[0], p[0]))
    raw = torch.empty(cout, cin, *k, dtype=torch.float64)
    tail = torch.empty_like(raw)
    m0 = (M - 1) // 32 * 32
    for r in range(k[0]):
        for t in range(k[1]):
            xs = xp[:, r * dil:r * dil + s[0] * (oh - 1) + 1:s[0], t * dil:t * dil + s[1] * (ow - 1) + 1:s[1], :].reshape(M, cin)
            raw[:, :, r, t] = g.t() @ xs
            tail[:, :, r, t] = g[m0:].t() @ xs[m0:]
    return raw, tail


_CACHE = {}


def _operands(row):
    """host operands and the fp64 reference of a row (cached: the three modes of a row share them)"""
    if row["name"] in _CACHE:
        return _CACHE[row["name"]]
    _CACHE.clear()
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row)
    M = nb * oh * ow
    gen = torch.Generator().manual_seed(sum(map(ord, row["name"])))
    img = None
    if row.get("u8"):
        img = torch.randint(0, 256, (nb, cin, h, w), dtype=torch.uint8, generator=gen)
        x = O.prep_images(img.float()).bfloat16().permute(0, 2, 3, 1).contiguous()
    else:
        x = torch.randn(nb, h, w, cin, generator=gen)
    gz = torch.randn(nb, oh, ow, cout, generator=gen)
    if row["dtype"] == "bf16":
        x, gz = x.bfloat16(), gz.bfloat16()
    raw, tail = wgrad_reference(x.double(), gz.reshape(M, cout).double(), k, s, p, dil, oh, ow)
    g64 = gz.reshape(M, cout).double()
    op = dict(x=x, gz=gz, img=img, raw=raw, tail=tail, colsum=g64.sum(0), colabs=g64.abs().sum(0),
              scale=torch.rand(cout, generator=gen) + 0.5, w=torch.randn(cout, cin, *k, generator=gen), M=M, oh=oh, ow=ow)
    op["dw_pre"] = torch.randn(cout, cin, *k, generator=gen) * float(raw.std())
    op["db_pre"] = torch.randn(cout, generator=gen) * float(op["colsum"].abs().max())
    op["wdot_pre"] = torch.randn(cout, generator=gen) * float((op["w"].double() * raw).sum((1, 2, 3)).abs().max())
    _CACHE[row["name"]] = op
    return op


def _view(t, dtype, ld, off, cpad):
    """[nb][h][w][c] host tensor -> device NHWC view: channels [off, off + c) hold t, [off + c, off + cpad) zeros (the chunk padding the
    kernels may read), every other channel of the pixel stride POISON"""
    *lead, c = t.shape
    buf = torch.full((*lead, ld), POISON, dtype=dtype)
    buf[..., off:off + cpad] = 0
    buf[..., off:off + c] = t.to(dtype)
    return buf.cuda()


def _guarded(n):
    buf = torch.full((n + 2 * NG,), GUARD, dtype=torch.float32, device="cuda")
    return buf, buf[NG:NG + n]


def _channel_err(got, want, terms):
    """max over channels of |err| / sum |terms| (immune to cancellation in the sum)"""
    return Measured(((got.double().cpu() - want).abs() / terms.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row", WGRAD_CASES, ids=[r["name"] for r in WGRAD_CASES])
def test_wgrad_kernel_against_fp64(env, row, mode, monkeypatch):
    lib, L, nhwc, ops = env
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row)
    ldi, cioff, ldo, cooff = row["ld"]
    fp32 = row["dtype"] == "fp32"
    epc = 4 if fp32 else 8
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, cin, oh, ow, cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = k[0], k[1], s[0], s[1], p[0], p[1], dil, dil
    d.ldi, d.cioff, d.ldo, d.cooff = ldi, cioff, ldo, cooff
    d.dtype, d.in_u8 = (L.DIN_F32 if fp32 else L.DIN_BF16), int(bool(row.get("u8")))
    names = C.create_string_buffer(512)
    assert 0 < lib.din_conv_kernel_names(C.byref(d), 2, 0, 0, 0, names, len(names)) <= len(names), L.load().din_last_error_string()
    assert names.value.decode().split("\n")[0] == row["kernel"], f"{row['name']}: the planner picked {names.value.decode().split()[0]}"
    bm, bn = C.c_int32(0), C.c_int32(0)
    L.check(lib.din_conv_kernel_tile(C.byref(d), 2, C.byref(bm), C.byref(bn)))
    assert (bm.value, bn.value) == row["code"], f"{row['name']}: planner picked kernel code {(bm.value, bn.value)}, not {row['kernel']}"
    wsb = lib.din_conv_workspace_bytes(C.byref(d), 2)
    if "slices" in row:                                     # (two-workgroups-per-CU kernel: [slices][cout_pad][kcols_pad] fp32 partials)
        slices = wsb // (_pad(_pad(cout, row["code"][0]), 128) * _pad(k[0] * k[1] * _pad(cin, epc), 128) * 4)
        assert row["slices"][0] <= slices <= row["slices"][1], f"{row['name']}: {slices} slices"
    if row.get("u8"):
        assert lib.din_conv_accepts_u8(C.byref(d)) == 1
    if row.get("direct"):                                   # one slice: [1][cout_pad][kcols_pad] fp32 partials (+ pacing words)
        assert wsb < 2 * _pad(_pad(cout, row["code"][0]), 128) * _pad(k[0] * k[1] * cin, 256) * 4, f"{row['name']}: more than one slice"

    op = _operands(row)
    raw, M = op["raw"], op["M"]
    bar = BAR[row["dtype"]]
    # the bar bites: a kernel that lost the last 32-pixel stage of M would fail it by >= 10x
    assert float(rel(raw - op["tail"], raw)) >= 10 * bar, f"{row['name']}: dropping the last stage moves dW by less than 10x the bar"

    tdt = torch.float32 if fp32 else torch.bfloat16
    xin = op["img"].cuda() if row.get("u8") else _view(op["x"], tdt, ldi, cioff, _pad(cin, epc))
    gin = _view(op["gz"], tdt, ldo, cooff, _pad(cout, 8))
    scale_d, w_d = op["scale"].cuda(), op["w"].cuda()
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    ndw = cout * cin * k[0] * k[1]
    dw_buf, dw = _guarded(ndw)
    db_buf, db = _guarded(cout)
    wd_buf, wdot = _guarded(cout)
    scale64, w64 = op["scale"].double()[:, None, None, None], op["w"].double()
    dot = (w64 * raw).sum((1, 2, 3))
    dot_abs = (w64 * raw).abs().sum((1, 2, 3))
    nan = float("nan")
    if mode == "plain":
        pre = (nan, nan, nan)
        want_dw, want_db, want_wd = raw, op["colsum"], None
        terms_db, terms_wd = op["colabs"], None
        args = (None, None, None, 0)
    elif mode == "production":
        pre = (nan, op["db_pre"], op["wdot_pre"])
        want_dw = scale64 * raw
        want_db, want_wd = op["db_pre"].double() + op["colsum"], op["wdot_pre"].double() + dot
        terms_db, terms_wd = op["colabs"] + op["db_pre"].double().abs(), dot_abs + op["wdot_pre"].double().abs()
        args = (scale_d.data_ptr(), w_d.data_ptr(), wdot.data_ptr(), 2)
    else:
        pre = (op["dw_pre"], nan, nan)
        want_dw = op["dw_pre"].double() + scale64 * raw
        want_db, want_wd = op["colsum"], dot
        terms_db, terms_wd = op["colabs"], dot_abs
        args = (scale_d.data_ptr(), w_d.data_ptr(), wdot.data_ptr(), 1)

    def launch():
        ws.fill_(0x7f)
        for t, v in zip((dw, db, wdot), pre):
            t.copy_(v.reshape(t.shape)) if torch.is_tensor(v) else t.fill_(v)
        L.check(lib.din_conv_wgrad(C.byref(d), xin.data_ptr(), gin.data_ptr(), dw.data_ptr(), db.data_ptr(), *args, ws.data_ptr(), wsb, None))
        torch.cuda.synchronize()

    for _ in range(2):
        launch()
        for buf, n in ((dw_buf, ndw), (db_buf, cout), (wd_buf, cout)):
            assert bool((buf[:NG] == GUARD).all()) and bool((buf[NG + n:] == GUARD).all()), f"{row['name']}: wrote outside an output"
        assert rel(dw.reshape(raw.shape), want_dw) <= bar
        assert _channel_err(db, want_db, terms_db) <= BAR_BIAS
        if want_wd is not None:
            assert _channel_err(wdot, want_wd, terms_wd) <= bar
        else:
            assert bool(wdot.isnan().all()), f"{row['name']}: wdot written without being asked for"

    if row.get("direct") and mode == "plain":
        # the single-slice 1x1 launch writes dW from the pipelined kernel's accumulators: bit-identical to its partial buffer + reduce form
        got = dw.clone(), db.clone()
        monkeypatch.setenv("DIN_WGRAD_DIRECT", "0")
        launch()
        assert torch.equal(dw, got[0]), "direct-to-dW epilogue and the reduce launch disagree"
        assert torch.equal(db, got[1])
