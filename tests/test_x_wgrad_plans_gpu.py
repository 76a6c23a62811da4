"""Direct fp64 checks of the conv weight gradients in the launch plans the training workload
runs in, through the C ABI: several patches per block with short and exact last splits, 16 / 17
/ 33 splits (one- and two-pass reduction), both M-subtile counts, two sources with up2,
cout_store < Cout, ragged channel blocks (the 3x3 / stride-1 fast path: tcam_conv_wgrad_s2_f16x3,
_s3_f16x3, _s3 on the bf16 and on the fp32 MFMA, _s1), and the generic kernel with several
pixel splits and a K-step tail (tcam_conv_wgrad_s3s2 and the fall-through of _s3 / _s1), and
wgrad11 with three splits, a short last one and a last pixel chunk of 9 in each of its four
<wm, wn> variants (the checks of tests/test_gpu_enc_train.py at wgrad_ref.W11_CASES).  Cases,
plans, reference and bounds: tests/wgrad_ref.py (pinned by tests/test_wgrad_ref.py); every case
asserts the plan it was chosen for.  Operands are the values the device stored; dy spreads over
logspace(-2, 2) per channel (times 1e-7 again for the f16x3 entry points) with one all-zero dy
and one all-zero x channel; dW and the workspace are filled with NaN before the call, a NaN
guard region behind dW must stay NaN, and every call is made twice and compared bit for bit.
Bounds, elementwise: 1e-6 mag (f16x3, x6, fp32 MFMA, generic), 2^-11 |ref| + 2e-6 (mag + 1e-3)
with an fp16-valued dW (S1).

Measured on an MI355X, worst error / bound over the cases (the whole file runs in 4 s): 3x3
s2_f16x3 0.054, s3_f16x3 0.054 (both at splits 16 / 17, dy x 1e-7), s3 x6 0.055 and s3 fp32 MFMA
0.061 (6 patches per block), S1 0.956 (fp16's half ulp); with 2 patches per block and 33 splits
0.025 .. 0.032, the seg-head form 0.022 .. 0.038; generic s3s2 0.102, s3 0.110 (3x3 / 2), S1
0.921.  No plan comes near the 0.3 that tests/test_grad_chain_gpu.py records at one patch per
block on its 198-pixel sums.

Measured once against deliberately wrong builds of csrc/train.hip (wrong sums only): with
wgrad33x6_kernel stopping after a split's first patch, with its last split one patch short when
that split holds several, and with wgrad_kernel skipping the first pixel of every split but the
first, each of the 175 direct weight-gradient tests the suite had before passes; here 30, 12 and
9 tests fail — every x6 / f16x3 / S1 entry point of the cases with two or more patches per
block, of ppb6_one_pass and thin8_exact_last, and every generic case."""
import pytest
import torch

import wgrad_ref as R
from tcam_wsol_video_amd import _lib
from test_gpu_enc_train import (_act, _dy_scaled, _nchw, _st, check_wgrad11_amp,
                                check_wgrad11_f16x3)
from test_x_train_fwd_gpu import _report, _twice

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 1024                       # floats behind dW that no kernel may write
FMT = {"s3": "x6", "s2": "f16x3", "s1": "amp"}
# entry point -> (operand layout, the dy scales it runs at)
ENTRIES33 = {"s2_f16x3": ("s2", (1.0, 1e-7)), "s3_f16x3": ("s3", (1.0, 1e-7)),
             "s3_x6": ("s3", (1.0,)), "s3_fp32": ("s3", (1.0,)), "s1": ("s1", (1.0,))}
ENTRIES_G = {"s3s2": ("s3", "s2"), "s3": ("s3", "s3"), "s1": ("s1", "s1")}   # (dy, x) layouts

_cache = {}


def _operands33(cuda, name, lay, dmag):
    """The stored operands of a 3x3 case in one layout, with the fp64 reference on them:
    computed once per (case, layout, scale) and shared by the entry points that read them."""
    key = (name, lay, dmag)
    if key not in _cache:
        c = R.W33_CASES[name]
        H, W, _ = R.w33_dims(c)
        xs, dy = R.wgrad_inputs(c["B"], c["cout"], [s[:3] for s in c["srcs"]], (H, W), dmag,
                                seed=len(name) + c["cout"])
        xt = [_act(x, cuda, FMT[lay]) for x in xs]
        o = dict(x=xt)
        if lay == "s2":   # the trainer's form: the per-channel scaled S2 copy of an S3 dy
            o["dy"], o["scale"] = _dy_scaled(_act(dy, cuda, "x6"))
            d64 = _nchw(o["dy"]) / o["scale"].double().cpu()[None, :, None, None]
        else:
            o["dy"] = _act(dy, cuda, FMT[lay])
            d64 = _nchw(o["dy"])
        assert (d64[:, R.ZERO_DY_CH] == 0).all() and (d64.abs().amax((0, 2, 3)) > 0).sum() == \
            c["cout"] - 1
        o["ref"], o["mag"] = R.wgrad_ref([(_nchw(t), s[3]) for t, s in zip(xt, c["srcs"])], d64,
                                         3, 1, 1)
        _cache[key] = o
    return _cache[key]


def _src_array(tensors, shapes, stride=1):
    arr = (_lib.tcam_conv_src * len(tensors))()
    for i, (t, (C, h, w, up2)) in enumerate(zip(tensors, shapes)):
        arr[i] = _lib.tcam_conv_src(t.data_ptr(), C, h, w, stride, up2)
    return arr


def _nan_bytes(n, dev):
    """A workspace whose every float is NaN: a partial sum read before it was written shows."""
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)


def _call(entry, arr, nsrc, B, dy, scale, cout, Ho, Wo, k, pad, cout_store, n_dw, nb):
    """One call of a conv wgrad entry point on a NaN dW (+ guard) and a NaN workspace; returns
    (dw with its guard, overflow flag)."""
    lib = _lib.load()
    dev = dy.device
    ws = _nan_bytes(nb, dev)
    dw = torch.full((n_dw + GUARD,), NAN, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    head = (arr, nsrc, B, dy.data_ptr())
    tail = (cout, Ho, Wo, k[0], k[1], pad[0], pad[1], cout_store, dw.data_ptr(), ws.data_ptr(),
            nb)
    if entry == "s2_f16x3":
        rc = lib.tcam_conv_wgrad_s2_f16x3(*head, scale.data_ptr(), *tail, _st())
    elif entry == "s3_f16x3":
        rc = lib.tcam_conv_wgrad_s3_f16x3(*head, *tail, flag.data_ptr(), _st())
    elif entry == "s3_fp32":
        lib.tcam_wgrad_force_fp32(1)
        try:
            rc = lib.tcam_conv_wgrad_s3(*head, *tail, _st())
        finally:
            lib.tcam_wgrad_force_fp32(0)
    else:
        fn = {"s3_x6": "tcam_conv_wgrad_s3", "s3": "tcam_conv_wgrad_s3",
              "s1": "tcam_conv_wgrad_s1", "s3s2": "tcam_conv_wgrad_s3s2"}[entry]
        rc = getattr(lib, fn)(*head, *tail, _st())
    assert rc == 0, (entry, rc)
    return dw, flag


def _check(tag, dw, flag, shape, ref, mag, s1):
    """dW against the reference within its bound; the guard intact; exact zeros where an
    operand channel is all zero; returns the worst error / bound."""
    n = ref.numel()
    assert int(flag) == 0, tag
    assert torch.isnan(dw[n:]).all(), tag + ": written behind dW"
    got = dw[:n].view(shape).double().cpu()
    assert torch.isfinite(got).all(), tag
    if shape[0] > R.ZERO_DY_CH:
        assert (got[R.ZERO_DY_CH] == 0).all(), tag
    if (mag[:, R.ZERO_X_CH] == 0).all():
        assert (got[:, R.ZERO_X_CH] == 0).all(), tag
    if s1:
        assert R.is_fp16(got), tag
    return R.ratio(got, ref, R.bound_s1(ref, mag) if s1 else R.bound_f32(mag))


def _run33(cuda, name, entry, dmag, scale_of=None):
    c = R.W33_CASES[name]
    plan = R.w33_case_plan(name)          # asserts the regime the case was chosen for
    H, W, ctot = R.w33_dims(c)
    o = _operands33(cuda, name, ENTRIES33[entry][0], dmag)
    store = c.get("cout_store", c["cout"])
    arr = _src_array(o["x"], c["srcs"])
    nb = int(_lib.load().tcam_conv_wgrad_ws_bytes(arr, len(c["srcs"]), c["B"], c["cout"], H, W,
                                                  3, 3))
    assert nb == plan["ws_bytes"]
    scale = o.get("scale")
    if scale_of is not None:
        scale = scale_of(scale)
    dw, flag = _twice(lambda: _call(entry, arr, len(c["srcs"]), c["B"], o["dy"], scale,
                                    c["cout"], H, W, (3, 3), (1, 1), store, store * ctot * 9, nb))
    return dw, flag, (store, ctot, 3, 3), o["ref"][:store], o["mag"][:store]


@pytest.mark.parametrize("entry,dmag", [(e, d) for e, (_, ds) in ENTRIES33.items() for d in ds])
@pytest.mark.parametrize("name", list(R.W33_CASES))
def test_wgrad33_in_every_plan_matches_fp64(cuda, name, entry, dmag):
    """The 3x3 / stride-1 weight gradient of every entry point at every case of
    wgrad_ref.W33_CASES (the plan each reaches is annotated and asserted there)."""
    dw, flag, shape, ref, mag = _run33(cuda, name, entry, dmag)
    tag = f"wgrad33 {name} {entry} dmag {dmag:g}"
    _report(tag, {"dW": _check(tag, dw, flag, shape, ref, mag, entry == "s1")})


def test_wgrad33_with_a_neighbours_scale_is_rejected(cuda):
    """Control on the device: the scales handed to tcam_conv_wgrad_s2_f16x3 rotated by one
    channel give a dW the checker rejects."""
    dw, flag, shape, ref, mag = _run33(cuda, "up2_skip_two_pass", "s2_f16x3", 1.0,
                                       scale_of=lambda s: s.roll(1).contiguous())
    got = dw[:ref.numel()].view(shape).double().cpu()
    assert not R.accept(got, ref, R.bound_f32(mag))


def _operands_g(cuda, name, ldy, lx):
    key = (name, ldy, lx)
    if key not in _cache:
        c = R.WG_CASES[name]
        xs, dy = R.wgrad_inputs(c["B"], c["cout"], [(c["cin"], c["H"], c["W"])], R.wg_dims(c),
                                1.0, seed=len(name))
        o = dict(x=_act(xs[0], cuda, FMT[lx], c["cpad"]), dy=_act(dy, cuda, FMT[ldy]))
        x64 = _nchw(o["x"])
        assert x64.shape[1] == c["cpad"] and (x64[:, c["cin"]:] == 0).all()
        o["ref"], o["mag"] = R.wgrad_ref([(x64, 0)], _nchw(o["dy"]), c["k"], c["stride"],
                                         c["pad"])
        _cache[key] = o
    return _cache[key]


@pytest.mark.parametrize("entry", list(ENTRIES_G))
@pytest.mark.parametrize("name", list(R.WG_CASES))
def test_generic_wgrad_with_pixel_splits_matches_fp64(cuda, name, entry):
    """wgrad_kernel + wgrad_reduce_kernel with several pixel splits, a short last split and a
    K-step tail (wgrad_ref.WG_CASES): tcam_conv_wgrad_s3s2 (dy S3, x S2) and the fall-through of
    tcam_conv_wgrad_s3 and tcam_conv_wgrad_s1."""
    lib = _lib.load()
    c = R.WG_CASES[name]
    plan = R.wg_case_plan(name)
    Ho, Wo = R.wg_dims(c)
    o = _operands_g(cuda, name, *ENTRIES_G[entry])
    arr = _src_array([o["x"]], [(c["cpad"], c["H"], c["W"], 0)], c["stride"])
    query = lib.tcam_conv_wgrad_generic_ws_bytes if entry == "s3s2" else \
        lib.tcam_conv_wgrad_ws_bytes
    nb = int(query(arr, 1, c["B"], c["cout"], Ho, Wo, *c["k"]))
    assert nb == plan["ws_bytes"]
    shape = (c["cout"], c["cpad"], *c["k"])
    n = c["cout"] * c["cpad"] * c["k"][0] * c["k"][1]
    dw, flag = _twice(lambda: _call(entry, arr, 1, c["B"], o["dy"], None, c["cout"], Ho, Wo,
                                    c["k"], c["pad"], c["cout"], n, nb))
    tag = f"generic wgrad {name} {entry}"
    _report(tag, {"dW": _check(tag, dw, flag, shape, o["ref"], o["mag"], entry == "s1")})
    if c["cpad"] > c["cin"]:      # the padded image channels: exactly zero
        assert (dw[:n].view(shape)[:, c["cin"]:] == 0).all()


# --------------------------------------------------------------------------- wgrad11
W11_PARAMS = [pytest.param(s, w, id="-".join(map(str, s))) for s, w in R.W11_CASES]


@pytest.mark.parametrize("dmag", [1.0, 1e-7])
@pytest.mark.parametrize("shape,want", W11_PARAMS)
def test_wgrad11_f16x3_in_every_variant_matches_fp64(cuda, shape, want, dmag):
    """test_gpu_enc_train.test_wgrad11_f16x3_matches_fp64's check (1e-6 mag, dy down to 1e-7) at
    wgrad_ref.W11_CASES: (B, cin, cout, H, W, stride) with three splits of 11 / 11 / 9 chunks and
    a last chunk of 9 pixels, in the <1, 1>, <2, 2> (ragged), <2, 1> and <1, 2> kernels."""
    R.w11_case_plan(shape, want)
    check_wgrad11_f16x3(cuda, *shape, dmag)


@pytest.mark.parametrize("shape,want", W11_PARAMS)
def test_wgrad11_amp_in_every_variant_matches_fp64(cuda, shape, want):
    """test_gpu_enc_train.test_wgrad11_amp_matches_fp64's check (2^-11 |ref| + 1e-6 mag) at the
    same cases."""
    R.w11_case_plan(shape, want)
    check_wgrad11_amp(cuda, *shape)
