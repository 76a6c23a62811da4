"""The weight-pack entries (tcam_pack_weight_x6 / _f16 / _f16x3 and the batched
tcam_pack_weights) against a host reference written from include/tcam_hip.h's statement of
the format, bit for bit:

  selection   Wsel[k][m], k = tap * Cin' + c'.  mode 0: W[m][c'][kh][kw], Cin' = max(CtotW,
              cin_pad).  mode 1: W[c'][c0 + m][KH-1-kh][KW-1-kw] over m < cout_sel, Cin' =
              max(CoutW, cin_pad).  Rows beyond the weight's channels, up to Kpad = roundup(K,
              32), and columns up to Mpad = roundup(Cout', 32), are zero.  kdiv (f16x3): a power
              of two per input channel c' that the weights are divided by.
  parts       x6: hi = rne_bf16(v), mid = rne_bf16(v - hi), lo = rne_bf16(v - hi - mid);
              fp16: rne_f16(v); f16x3: u = v / s_m, h = rne_f16(u), l = rne_f16(u - h), s_m the
              power of two with max_k |v| / s_m in [2^14, 2^15) (exponent >= -126; 1 for an
              all-zero column).
  layout      out[kt][g][part][m][e] = part of Wsel[32 kt + 8 g + e][m].

Output and scale buffers are pre-filled with a sentinel, so the padding rows and columns are
shown to be written (zero, scale 1).  Every case has one all-zero column and one column
whose maximum is exactly a power of two.
"""
import pytest
import torch

from tcam_wsol_video_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
FMTS = ("x6", "f16", "f16x3")

# (CoutW, CtotW, KH, KW), mode, c0, sel, cin_pad, kdiv?
CASES = {
    "k_not_32": ((40, 24, 1, 1), 0, 0, 0, 0, False),       # K = 24
    "stem": ((64, 3, 7, 7), 0, 0, 0, 8, False),            # input channels padded 3 -> 8
    "seg_head": ((2, 16, 3, 3), 1, 0, 16, 8, False),       # dy padded past CoutW
    "dgrad_kdiv": ((24, 40, 3, 3), 1, 8, 16, 0, True),     # a channel slice, dy's scales
}
# the other two items of the batched table (first and last: the case's blocks start past 0)
FILLERS = (((8, 8, 1, 1), 0, 0, 0, 0, False), ((16, 8, 3, 3), 1, 0, 8, 0, False))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _roundup(v, m):
    return (v + m - 1) // m * m


def _weight(spec, seed):
    """(w, kdiv) on the host: column 1 of Wsel all zero, column 0 with a power-of-two maximum."""
    (co, ci, kh, kw), mode, c0, sel, cpad, has_kdiv = spec
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(co, ci, kh, kw, generator=g) * 0.1
    kdiv = 2.0 ** torch.randint(-3, 4, (co if mode else ci,), generator=g).float() \
        if has_kdiv else None
    col = (lambda m: w[m]) if mode == 0 else (lambda m: w[:, c0 + m])
    col(1).zero_()
    if has_kdiv:   # one entry: 0.25 / kdiv is the column's maximum, a power of two
        col(0).zero_()
        col(0)[0, 0, 0] = 0.25
    else:
        col(0).clamp_(-0.2, 0.2)
        col(0)[0, 0, 0] = -0.25
    return w, kdiv


def _wsel(spec, w, kdiv):
    """Wsel (Kpad, Mpad) fp32, zero padded."""
    (co, ci, kh, kw), mode, c0, sel, cpad, _ = spec
    if mode == 0:
        v = w.permute(2, 3, 1, 0)                                  # [kh][kw][c'][m]
        cinp, coutp = max(ci, cpad), co
    else:
        v = w[:, c0:c0 + sel].flip(2, 3).permute(2, 3, 0, 1)       # [kh][kw][c'][m]
        cinp, coutp = max(co, cpad), sel
    if kdiv is not None:
        v = v / kdiv.view(1, 1, -1, 1)
    K = kh * kw * cinp
    kp, mp = _roundup(K, 32), _roundup(coutp, 32)
    assert (kp, mp) == ops.conv_x6_weight_dims(K, coutp)
    full = torch.zeros(kh, kw, cinp, mp)
    full[:, :, :v.shape[2], :coutp] = v
    out = torch.zeros(kp, mp)
    out[:K] = full.reshape(K, mp)
    return out


def _expected(spec, w, kdiv, fmt):
    """(operand as int16 (Kpad/32, 4, parts, Mpad, 8), scales (Mpad,) or None)."""
    v = _wsel(spec, w, kdiv)
    kp, mp = v.shape
    scale = None
    if fmt == "x6":
        hi = v.to(torch.bfloat16)
        r1 = v - hi.float()
        mid = r1.to(torch.bfloat16)
        parts = [hi, mid, (r1 - mid.float()).to(torch.bfloat16)]
    elif fmt == "f16":
        parts = [v.to(torch.float16)]
    else:
        t = v.abs().amax(0)
        _, ex = torch.frexp(t)                       # t in [2^(ex-1), 2^ex)
        scale = torch.where(t > 0, torch.ldexp(torch.ones(mp), (ex - 15).clamp(min=-126)),
                            torch.ones(mp))
        u = v / scale
        h = u.to(torch.float16)
        parts = [h, (u - h.float()).to(torch.float16)]
    p = torch.stack([q.view(torch.int16) for q in parts])         # [part][k][m]
    p = p.view(len(parts), kp // 32, 4, 8, mp).permute(1, 2, 0, 4, 3).contiguous()
    return p, scale


def _buffers(exp, scale, dev):
    out = torch.full(exp.shape, SENTINEL, dtype=torch.int16, device=dev)
    sc = torch.full((exp.shape[3],), -7.0, device=dev) if scale is not None else None
    return out, sc


def _item(it, spec, w, kdiv, out, sc):
    (co, ci, kh, kw), mode, c0, sel, cpad, _ = spec
    it.w, it.out = w.data_ptr(), out.data_ptr()
    it.wscale = sc.data_ptr() if sc is not None else None
    it.kdiv = kdiv.data_ptr() if kdiv is not None else None
    it.mode, it.CoutW, it.CtotW, it.KH, it.KW = mode, co, ci, kh, kw
    it.c0, it.cout_sel, it.cin_pad = c0, sel, cpad


def _check(out, sc, exp, scale, what):
    assert torch.equal(out.cpu(), exp), f"{what}: packed operand differs"
    if scale is not None:
        assert torch.equal(sc.cpu(), scale), f"{what}: column scales differ"


@pytest.mark.parametrize("case,fmt", [(c, f) for c in CASES for f in FMTS
                                      if f == "f16x3" or not CASES[c][5]])
def test_pack_entries_match_host_reference(cuda, case, fmt):
    """The single entry of ``fmt`` and (fp16, f16x3) tcam_pack_weights over a three-item table
    with the case in the middle: operand and scales equal the host reference bit for bit,
    padding included."""
    lib = _lib.load()
    specs = [FILLERS[0], CASES[case], FILLERS[1]]
    host = [_weight(s, 100 + i) for i, s in enumerate(specs)]
    dev = [(w.to(cuda), k.to(cuda) if k is not None else None) for w, k in host]
    exps = [_expected(s, w, k, fmt) for s, (w, k) in zip(specs, host)]
    # the inputs are what they claim: column 0's maximum a power of two, column 1 all zero
    v = _wsel(specs[1], *host[1])
    assert torch.frexp(v[:, 0].abs().max())[0] == 0.5 and not v[:, 1].any()
    (co, ci, kh, kw), mode, c0, sel, cpad, _ = specs[1]
    (w, kdiv), (exp, scale) = dev[1], exps[1]
    out, osc = _buffers(exp, scale, cuda)
    if fmt == "f16x3":
        rc = lib.tcam_pack_weight_f16x3(w.data_ptr(), out.data_ptr(), osc.data_ptr(), mode, co,
                                        ci, kh, kw, c0, sel, cpad,
                                        kdiv.data_ptr() if kdiv is not None else None, _st())
    else:
        fn = lib.tcam_pack_weight_x6 if fmt == "x6" else lib.tcam_pack_weight_f16
        rc = fn(w.data_ptr(), out.data_ptr(), mode, co, ci, kh, kw, c0, sel, cpad, _st())
    assert rc == 0
    _check(out, osc, exp, scale, f"{case} {fmt} single")
    if fmt == "x6":
        return   # no batched x6 pack
    items = (_lib.tcam_pack_item * 3)()
    bufs = [_buffers(e, s, cuda) for e, s in exps]
    for it, s, (w, k), (o, c) in zip(items, specs, dev, bufs):
        _item(it, s, w, k, o, c)
    table = torch.empty(int(lib.tcam_pack_table_bytes(3)), dtype=torch.uint8, device=cuda)
    assert lib.tcam_pack_weights(items, 3, 1 if fmt == "f16x3" else 0, table.data_ptr(),
                                 _st()) == 0
    for i, ((o, c), (e, s)) in enumerate(zip(bufs, exps)):
        _check(o, c, e, s, f"{case} {fmt} batched item {i}")
