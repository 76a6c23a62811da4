"""CPU checks of tests/wgrad_ref.py, the reference, bounds, plan restatements and case table of
the conv weight gradients' kernel tests (tests/test_x_wgrad_plans_gpu.py): the reference pinned
to torch's own fp64 conv2d_weight; the restated planners tied to the C++ through the workspace
sizes of the built library (which loads without a device); every case asserts the plan it was
chosen for; and the bounds' teeth — an fp32 emulation of each case's split sum is accepted, and
the same emulation with the tail patch of the last split dropped, one pixel dropped, one split
counted twice or a neighbouring channel's dy scale is rejected."""
import ctypes

import pytest
import torch

import wgrad_ref as R
from tcam_wsol_video_amd import _lib

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------ the reference
# (srcs (C, h, w, up2), cout, k, stride, pad)
REF_CASES = [
    ([(8, 6, 7, 0)], 5, 3, 1, 1),
    ([(4, 3, 5, 1), (6, 6, 10, 0)], 3, 3, 1, 1),
    ([(6, 9, 11, 0)], 4, 3, 2, 1),
    ([(3, 13, 10, 0)], 4, 7, 2, 3),
    ([(5, 6, 9, 0)], 2, (1, 7), 1, (0, 3)),
    ([(7, 9, 8, 0)], 6, 1, 2, 0),
    ([(4, 2, 3, 1), (2, 4, 6, 0)], 3, 3, 2, 1),
]


@pytest.mark.parametrize("srcs,cout,k,stride,pad", REF_CASES)
def test_wgrad_ref_equals_torch_conv2d_weight(srcs, cout, k, stride, pad):
    g = torch.Generator().manual_seed(len(srcs) + cout)
    B = 2
    xs = [(torch.randn(B, C, h, w, generator=g, dtype=F64), up2) for (C, h, w, up2) in srcs]
    x = R.cat_sources(xs)
    (KH, KW), (ph, pw) = R._pair(k), R._pair(pad)
    Ho, Wo = (x.shape[2] + 2 * ph - KH) // stride + 1, (x.shape[3] + 2 * pw - KW) // stride + 1
    dy = torch.randn(B, cout, Ho, Wo, generator=g, dtype=F64)
    ref, mag = R.wgrad_ref(xs, dy, k, stride, pad)
    shape = (cout, x.shape[1], KH, KW)
    want = torch.nn.grad.conv2d_weight(x, shape, dy, stride=stride, padding=(ph, pw))
    wmag = torch.nn.grad.conv2d_weight(x.abs(), shape, dy.abs(), stride=stride, padding=(ph, pw))
    assert ref.shape == want.shape
    assert ((ref - want).abs() <= 1e-13 * wmag).all()
    assert ((mag - wmag).abs() <= 1e-13 * wmag).all() and (mag >= ref.abs() - 1e-13 * wmag).all()


def test_wgrad_inputs_conditions():
    xs, dy = R.wgrad_inputs(2, 16, [(8, 5, 6), (8, 5, 6)], (5, 6), 1e-7, 3)
    assert (xs[0][:, R.ZERO_X_CH] == 0).all() and (dy[:, R.ZERO_DY_CH] == 0).all()
    amax = dy.abs().amax((0, 2, 3))
    live = [c for c in range(16) if c != R.ZERO_DY_CH]
    assert (amax[live] > 0).all() and amax[15] / amax[0] > 1e3 and amax[15] < 1e-4
    assert torch.equal(R.wgrad_inputs(3, 8, [(3, 9, 9)], (5, 5), 1.0, 1)[1][:, R.ZERO_DY_CH],
                       torch.zeros(3, 5, 5))


# ------------------------------------------------------------------ plans
def test_every_case_reaches_the_plan_it_was_chosen_for():
    cov = R.coverage()   # asserts each case's plan
    assert cov["ppb"] == {1, 2, 3} and cov["last"] == {"short", "exact"}
    assert {16, 17} <= cov["splits"] and cov["msub"] == {1, 2} and cov["passes"] == {False, True}
    assert cov["generic_tail"]
    assert cov["w11"] == {(1, 1), (2, 2), (2, 1), (1, 2)}
    # what the suite tested before: one patch per block, one generic split, at most a full tail
    for B, cout, srcs in R.W33_OLD:
        C, h, w, up2 = srcs[0]
        assert R.w33_plan(B, cout, srcs, *((2 * h, 2 * w) if up2 else (h, w)))["ppb"] == 1
    assert all(R.wg_plan(*g)["splits"] == 1 for g in R.WG_OLD)
    for B, cin, cout, H, W, s in R.W11_OLD:
        p = R.w11_plan(B, cin, H, W, s, cout, (H - 1) // s + 1, (W - 1) // s + 1)
        assert p["splits"] == 1 or (p["tail"] == 0 and (p["wm"], p["wn"]) == (2, 2))


def test_split_pixels_partition_the_batch():
    for name, c in R.W33_CASES.items():
        H, W, _ = R.w33_dims(c)
        plan = R.w33_case_plan(name)
        sp = R.w33_split_pixels(plan, c["B"], H, W)
        assert len(sp) == plan["splits"]
        assert torch.equal(torch.cat(sp).sort().values, torch.arange(c["B"] * H * W)), name
    for name in R.WG_CASES:
        plan = R.wg_case_plan(name)
        assert torch.equal(torch.cat(R.wg_split_pixels(plan)), torch.arange(plan["P"]))
    for shape, want in R.W11_CASES:
        plan = R.w11_case_plan(shape, want)
        assert torch.equal(torch.cat(R.w11_split_pixels(plan)), torch.arange(plan["P"]))


def _src_array(srcs, stride=1):
    """tcam_conv_src[] with a non-null pointer that is never followed (the size queries only
    look at the shapes)."""
    buf = ctypes.create_string_buffer(16)
    arr = (_lib.tcam_conv_src * len(srcs))()
    for i, (C, h, w, up2) in enumerate(srcs):
        arr[i] = _lib.tcam_conv_src(ctypes.addressof(buf), C, h, w, stride, up2)
    return arr, buf


def test_restated_workspace_sizes_equal_the_library():
    lib = _lib.load()
    geoms = [(c["B"], c["cout"], c["srcs"]) for c in R.W33_CASES.values()] + R.W33_OLD
    for B, cout, srcs in geoms:
        C, h, w, up2 = srcs[0]
        H, W = (2 * h, 2 * w) if up2 else (h, w)
        arr, keep = _src_array(srcs)
        got = int(lib.tcam_conv_wgrad_ws_bytes(arr, len(srcs), B, cout, H, W, 3, 3))
        assert got == R.w33_plan(B, cout, srcs, H, W)["ws_bytes"] > 0, (B, cout, srcs)
        assert got == R.conv_wgrad_ws_bytes(B, cout, srcs, H, W, 3, 3)
    generic = [(c["B"], c["cout"], c["cpad"], *R.wg_dims(c), *c["k"], c["H"], c["W"], c["stride"])
               for c in R.WG_CASES.values()]
    generic += [(3, 16, 32, 6, 6, 3, 3, 12, 12, 2), (2, 64, 8, 20, 18, 7, 7, 40, 36, 2),
                (2, 48, 32, 7, 8, 3, 3, 14, 15, 2)]
    assert [g[:7] for g in generic[len(R.WG_CASES):]] == R.WG_OLD
    for B, cout, ctot, Ho, Wo, KH, KW, H, W, s in generic:
        arr, keep = _src_array([(ctot, H, W, 0)], s)
        want = R.wg_plan(B, cout, ctot, Ho, Wo, KH, KW)["ws_bytes"]
        assert int(lib.tcam_conv_wgrad_generic_ws_bytes(arr, 1, B, cout, Ho, Wo, KH, KW)) == want
        # the S3 / S1 entry points' fall-through sizes its workspace with the 3x3 query
        assert int(lib.tcam_conv_wgrad_ws_bytes(arr, 1, B, cout, Ho, Wo, KH, KW)) == want
        assert R.conv_wgrad_ws_bytes(B, cout, [(ctot, H, W, 0)], Ho, Wo, KH, KW) == want > 0
    for B, cin, cout, H, W, s in [c[0] for c in R.W11_CASES] + R.W11_OLD:
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        want = R.w11_plan(B, cin, H, W, s, cout, Ho, Wo)["ws_bytes"]
        assert int(lib.tcam_wgrad11_ws_bytes(B, cin, H, W, s, cout, Ho, Wo)) == want > 256


def test_size_queries_refuse_what_the_planners_refuse():
    lib = _lib.load()
    arr, keep = _src_array([(12, 8, 8, 0)])               # C % 8
    assert lib.tcam_conv_wgrad_ws_bytes(arr, 1, 2, 8, 8, 8, 3, 3) == 0
    assert R.conv_wgrad_ws_bytes(2, 8, [(12, 8, 8, 0)], 8, 8, 3, 3) == 0
    assert lib.tcam_wgrad11_ws_bytes(2, 8, 5, 5, 2, 8, 4, 3) == 0   # (Ho - 1) stride >= Hin
    assert R.w11_plan(2, 8, 5, 5, 2, 8, 4, 3) is None
    # two sources whose first does not end on a 32-channel block: the generic path
    srcs = [(16, 8, 8, 0), (16, 8, 8, 0)]
    arr, keep = _src_array(srcs)
    assert R.w33_plan(2, 8, srcs, 8, 8) is None
    assert int(lib.tcam_conv_wgrad_ws_bytes(arr, 2, 2, 8, 8, 8, 3, 3)) == \
        R.wg_plan(2, 8, 32, 8, 8, 3, 3)["ws_bytes"]
    # ... as test_wgrad_matches_fp64's up2 + skip geometry with a 16-channel first source is
    srcs = [(16, 5, 6, 1), (8, 10, 12, 0)]
    arr, keep = _src_array(srcs)
    assert int(lib.tcam_conv_wgrad_ws_bytes(arr, 2, 3, 32, 10, 12, 3, 3)) == \
        R.conv_wgrad_ws_bytes(3, 32, srcs, 10, 12, 3, 3) == \
        R.wg_plan(3, 32, 24, 10, 12, 3, 3)["ws_bytes"] > 0


# ------------------------------------------------------------------ teeth
def dy_scales(d):
    """dy_scale_kernel: per channel 2^k with max |dy| 2^k in [2^14, 2^15), 2^126 for an all-zero
    channel.  d: (P, Cout)."""
    amax = d.abs().amax(0)
    ex = torch.frexp(amax)[1].double()
    return torch.where(amax == 0, torch.tensor(2.0 ** 126, dtype=F64), 2.0 ** (15 - ex))


def emu_split_sum(d, taps, splits, scale=None, half=False, defect=None, tail=0):
    """The kernels' split sum in fp32: per split the fp32 sum over its pixels of dy x (dy times
    its channel's power-of-two scale when given), the splits summed in order — through chunk
    sums of 16 when there are more than 16, as reduce33 does — and the scale divided out; with
    ``half`` the operands are fp16 values and dW is rounded to fp16 (the AMP path).  d: (P,
    Cout) fp64, taps: [(P, C) fp64].  ``defect``: one of the wrong kernels (``tail``: the pixels
    of the last split's last patch / K-step / chunk)."""
    splits = [s.clone() for s in splits]
    if defect == "tail_patch":      # the last split stops one patch / K-step / chunk early
        splits[-1] = splits[-1][:-tail]
    elif defect == "pixel":         # an off-by-one inside a middle split
        k = len(splits) // 2
        splits[k] = splits[k][1:]
    ds = d * scale[None, :] if scale is not None else d
    d32 = ds.to(F32)
    assert torch.equal(d32.double(), ds)          # the operands are fp32 values
    out = []
    for xt in taps:
        x32 = xt.to(F32)
        parts = [d32[s].t() @ x32[s] for s in splits]
        if defect == "split_twice":
            parts.insert(1, parts[1])
        if len(parts) > R.K_RED_CHUNK:
            chunks = []
            for i in range(0, len(parts), R.K_RED_CHUNK):
                c = torch.zeros_like(parts[0])
                for p in parts[i:i + R.K_RED_CHUNK]:
                    c = c + p
                chunks.append(c)
            parts = chunks
        s = torch.zeros_like(parts[0])
        for p in parts:
            s = s + p
        if scale is not None:
            sc = scale.roll(-1) if defect == "neighbour_scale" else scale
            s = s / sc.to(F32)[:, None]
        out.append(s.half().double() if half else s.double())
    return torch.stack(out, 2)


def _regimes():
    for name in R.W33_CASES:
        yield "w33", name
    for name in R.WG_CASES:
        yield "wg", name
    for i in range(len(R.W11_CASES)):
        yield "w11", i


def _regime_operands(kind, key, dmag, half):
    """(d (P, co) fp64, taps [(P, c)], splits, tail) of a case on a subset of its channels (the
    columns of dW are independent; the pixel partition is the whole case's)."""
    q = (lambda t: t.half().float()) if half else (lambda t: t)
    if kind == "w33":
        c = R.W33_CASES[key]
        H, W, ctot = R.w33_dims(c)
        plan = R.w33_case_plan(key)
        xs, dy = R.wgrad_inputs(c["B"], c["cout"], [s[:3] for s in c["srcs"]], (H, W), dmag, 11)
        x = R.cat_sources([(q(v).double(), s[3]) for v, s in zip(xs, c["srcs"])])
        k, stride, pad = 3, 1, 1
        splits = R.w33_split_pixels(plan, c["B"], H, W)
        tail = len(R.w33_split_pixels(dict(plan, ppb=1, splits=plan["npatch"]), c["B"], H,
                                      W)[-1])
    elif kind == "wg":
        c = R.WG_CASES[key]
        plan = R.wg_case_plan(key)
        xs, dy = R.wgrad_inputs(c["B"], c["cout"], [(c["cin"], c["H"], c["W"])], R.wg_dims(c),
                                dmag, 12)
        x = q(xs[0]).double()
        k, stride, pad = c["k"], c["stride"], c["pad"]
        splits, tail = R.wg_split_pixels(plan), plan["tail"]
    else:
        (B, cin, cout, H, W, stride), want = R.W11_CASES[key]
        plan = R.w11_case_plan((B, cin, cout, H, W, stride), want)
        xs, dy = R.wgrad_inputs(B, cout, [(cin, H, W)], ((H - 1) // stride + 1,
                                                         (W - 1) // stride + 1), dmag, 13)
        x = q(xs[0]).double()
        k, pad = 1, 0
        splits, tail = R.w11_split_pixels(plan), plan["tail"]
    ch = sorted(set(range(min(8, x.shape[1]))) | set(range(max(0, x.shape[1] - 8), x.shape[1])))
    co = list(range(min(16, dy.shape[1])))
    dy64 = q(dy).double()[:, co]
    taps = list(R.tap_rows(x[:, ch], dy64.shape, k, stride, pad))
    ref, mag = R.wgrad_ref([(x[:, ch], 0)], dy64, k, stride, pad)
    return R.dy_rows(dy64), taps, splits, tail, ref.flatten(2), mag.flatten(2)


@pytest.mark.parametrize("dmag", [1.0, 1e-7])
@pytest.mark.parametrize("kind,key", list(_regimes()))
def test_bound_accepts_fp32_split_sum_and_rejects_defects(kind, key, dmag):
    """bound_f32 (1e-6 mag) on every case's own pixel partition, with the per-channel dy scales
    of the f16x3 kernels."""
    d, taps, splits, tail, ref, mag = _regime_operands(kind, key, dmag, False)
    assert len(splits) > 1 and tail > 0
    scale = dy_scales(d)
    assert len(set(scale.tolist())) > 2             # neighbouring channels differ somewhere
    bound = R.bound_f32(mag)
    good = emu_split_sum(d, taps, splits, scale)
    print(f"{kind} {key} dmag {dmag:g}: fp32 split sum at {R.ratio(good, ref, bound):.3g}")
    assert R.accept(good, ref, bound)
    assert R.accept(emu_split_sum(d, taps, splits), ref, bound)      # and unscaled
    for defect in ("tail_patch", "pixel", "split_twice", "neighbour_scale"):
        bad = emu_split_sum(d, taps, splits, scale, defect=defect, tail=tail)
        assert not R.accept(bad, ref, bound), defect


@pytest.mark.parametrize("kind,key", list(_regimes()))
def test_s1_bound_accepts_fp16_split_sum_and_rejects_defects(kind, key):
    """bound_s1 (2^-11 |ref| + 2e-6 (mag + 1e-3), dW an fp16 value) on fp16 operands."""
    d, taps, splits, tail, ref, mag = _regime_operands(kind, key, 1.0, True)
    bound = R.bound_s1(ref, mag)
    good = emu_split_sum(d, taps, splits, half=True)
    assert R.is_fp16(good) and R.accept(good, ref, bound)
    assert not R.is_fp16(emu_split_sum(d, taps, splits))             # fp32 sums are not fp16
    for defect in ("tail_patch", "pixel", "split_twice"):
        assert not R.accept(emu_split_sum(d, taps, splits, half=True, defect=defect,
                                          tail=tail), ref, bound), defect
