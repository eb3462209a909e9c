"""Python face of the C ABI (include/lfdm_hip.h): one thin function per entry point.

Tensors are torch fp32 tensors used only as device memory (data_ptr + current HIP stream);
all arithmetic happens in the HIP kernels of liblfdm_hip.so.  "CL" activations are 2-D tensors
(rows, C): rows = N*H*W pixels in (n, y, x) order, UNet frames n = b*T + t.
"""
import ctypes as C

import torch

from . import _native
from ._native import ConvParams, WarpParams

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_GELU = 0, 1, 2, 3, 4


def _lib():
    return _native.library()


def _stream(lib):
    if lib.kind == "hip":
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(lib, *tensors):
    for t in tensors:
        if t is None:
            continue
        if t.dtype not in (torch.float32, torch.int32):
            raise TypeError("lfdm ops take float32/int32 tensors, got %s" % t.dtype)
        if lib.kind == "hip" and not t.is_cuda:
            raise RuntimeError("lfdm ops need tensors on the GPU (no CPU fallback exists)")
        if lib.kind == "emu" and t.is_cuda:
            raise RuntimeError("emulation library needs CPU tensors")


def _ld(t):
    """Row stride of a row operand that goes to the library as a leading dimension (ld0, ldo, ldx, ss_ld, ...): the library walks a row
    with stride 1, so a transposed or column-strided view is refused here instead of being read as something else."""
    if t.dim() < 1 or t.stride(-1) != 1:
        raise ValueError("lfdm ops take row operands with adjacent columns (stride(-1) == 1) and a row stride, got strides %s"
                         % (tuple(t.stride()),))
    return t.stride(0)


def _dense(*tensors):
    """Operands whose entry point takes no leading dimension: the library addresses them as one dense block."""
    for t in tensors:
        if t is not None and not t.is_contiguous():
            raise ValueError("this lfdm op takes no row stride for this operand: a contiguous tensor is needed, got strides %s"
                             % (tuple(t.stride()),))


def empty(shape, like=None, device=None, dtype=torch.float32):
    dev = device if device is not None else like.device
    return torch.empty(shape, dtype=dtype, device=dev)


# ---------------------------------------------------------------------------------------------
# weight packing (one-time, load-time plumbing)
# ---------------------------------------------------------------------------------------------

def round_up(v, m):
    return (v + m - 1) // m * m


def _pack_k_major(wk, cout):
    """(K, cout) rows in k order -> [ceil(K/32)][coutp][32] (k contiguous per output channel)."""
    k = wk.shape[0]
    kp, coutp = round_up(k, 32), round_up(cout, 32)
    full = torch.zeros(kp, coutp, dtype=torch.float32, device=wk.device)
    full[:k, :cout] = wk
    return full.view(kp // 32, 32, coutp).permute(0, 2, 1).contiguous()


def pack_conv_weight(w):
    """(Cout, Cin, kh, kw) [or (Cout, Cin, 1, kh, kw) / (Cout, Cin)] -> lfdm_conv2d_cl_f32 layout:
    [ceil(K/32)][coutp][32], K = kh*kw*Cin flattened tap-major then channel."""
    if w.dim() == 5:
        w = w[:, :, 0]
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    return _pack_k_major(w.permute(2, 3, 1, 0).reshape(kh * kw * cin, cout), cout)


def pack_deconv_weight(w):
    """ConvTranspose3d weight (Cin, Cout, 1, 4, 4), stride 2, padding 1 -> four parity packs
    [(py, px, packed)]: output pixel (2q+py, 2q'+px) = 2x2 conv with pad (1-py, 1-px);
    tap ky' uses kernel row ky = 3 - 2ky' (py = 0) or 2 - 2ky' (py = 1)."""
    if w.dim() == 5:
        w = w[:, :, 0]
    cin, cout, kh, kw = w.shape
    assert kh == 4 and kw == 4
    packs = []
    for py in (0, 1):
        for px in (0, 1):
            kys = [3, 1] if py == 0 else [2, 0]
            kxs = [3, 1] if px == 0 else [2, 0]
            taps = [w[:, :, ky, kx] for ky in kys for kx in kxs]          # each (Cin, Cout)
            packs.append((py, px, _pack_k_major(torch.cat(taps, dim=0), cout)))
    return packs


def pack_deconv4_weight(w):
    """The four parity packs of pack_deconv_weight stacked in parity order q = 2*py + px: (4, chunks, coutp, 32), the
    `deconv4=` operand of conv_params (the whole ConvTranspose k4 s2 p1 as ONE launch)."""
    return torch.stack([pk for _, _, pk in pack_deconv_weight(w)]).contiguous()


def pack_conv_weight_dev(w, mode=0):
    """The packs of pack_conv_weight (mode 0), of the data-gradient filter w.transpose(0, 1).flip(-2, -1) (mode 1) and of
    pack_deconv4_weight (mode 2) built by ONE library launch (lfdm_pack_conv_weight_f32) - the training path re-packs every
    step.  w: (O, I, kh, kw), any strides on the two channel axes (a slice is not copied), the taps contiguous."""
    lib = _lib()
    _chk(lib, w)
    if w.dim() == 5:
        w = w[:, :, 0]
    if w.dim() == 2:
        w = w[:, :, None, None]
    n_o, n_i, kh, kw = w.shape
    taps = kh * kw
    if taps > 1 and (w.stride(3) != 1 or w.stride(2) != kw):
        w = w.contiguous()
    k = taps * n_i if mode == 0 else taps * n_o if mode == 1 else 4 * n_o
    n = n_o if mode == 0 else n_i
    shape = (round_up(k, 32) // 32, round_up(n, 32), 32)
    out = torch.empty(((4,) + shape) if mode == 2 else shape, dtype=torch.float32, device=w.device)
    lib.check(lib.lfdm_pack_conv_weight_f32(_p(w), n_o, n_i, taps, w.stride(0), w.stride(1), mode, _p(out), _stream(lib)),
              "lfdm_pack_conv_weight_f32")
    return out


def svd2x2_sym(a, b, c):
    """lfdm_svd2x2_sym_f32: (U (n,2,2), S (n,2)) of [[a, b], [b, c]] with LAPACK's sign convention."""
    lib = _lib()
    abc = torch.stack((a, b, c), dim=-1).float().contiguous()
    _chk(lib, abc)
    n = abc.shape[0]
    u = torch.empty(n, 2, 2, dtype=torch.float32, device=abc.device)
    s = torch.empty(n, 2, dtype=torch.float32, device=abc.device)
    lib.check(lib.lfdm_svd2x2_sym_f32(_p(abc), n, _p(u), _p(s), _stream(lib)), "lfdm_svd2x2_sym_f32")
    return u, s


def lfae_region_stats(logits, n, k, h, w, temperature):
    """lfdm_lfae_region_stats_f32 on the `regions` head's channels-last rows -> the RegionPredictor's output dict."""
    lib = _lib()
    _chk(lib, logits)
    dev = logits.device
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    heat, shift, covar, affine, u, d = e(n, k, h, w), e(n, k, 2), e(n, k, 2, 2), e(n, k, 2, 2), e(n * k, 2, 2), e(n * k, 2, 2)
    lib.check(lib.lfdm_lfae_region_stats_f32(_p(logits), _ld(logits), n, k, h, w, float(temperature), _p(heat), _p(shift),
                                             _p(covar), _p(affine), _p(u), _p(d), _stream(lib)), "lfdm_lfae_region_stats_f32")
    return {"shift": shift, "heatmap": heat, "covar": covar, "affine": affine, "u": u, "d": d}


def lfae_motion_inputs(src_img, driving, source, bg, frames, *, region_var, revert_axis_swap, use_covar, pad_to=32):
    """lfdm_lfae_motion_inputs_f32: -> (rows (N*h*w, ld) = the pixelwise-flow hourglass' channels-last input, sparse (N, K+1, h, w, 2)).
    src_img (B, 3, h, w); driving: dict of (N = B*frames, K, ...) tensors, source: dict of (B, K, ...) tensors."""
    lib = _lib()
    b, c, h, w = src_img.shape
    n = b * frames
    k = driving["shift"].shape[1]
    f = lambda t: None if t is None else t.detach().float().contiguous()
    img = f(src_img)
    dsh, ssh = f(driving["shift"]), f(source["shift"])
    dcv, scv = (f(driving["covar"]), f(source["covar"])) if use_covar else (None, None)
    daf, saf = (f(driving["affine"]), f(source["affine"])) if "affine" in driving else (None, None)
    bgm = f(bg)
    _chk(lib, img, dsh, ssh, dcv, scv, daf, saf, bgm)
    assert c == 3 and dsh.shape[0] == n and ssh.shape[0] == b
    ld = round_up(4 * (k + 1), pad_to)
    rows = torch.empty(n * h * w, ld, dtype=torch.float32, device=img.device)
    sparse = torch.empty(n, k + 1, h, w, 2, dtype=torch.float32, device=img.device)
    lib.check(lib.lfdm_lfae_motion_inputs_f32(_p(img), _p(dsh), _p(dcv), _p(daf), _p(ssh), _p(scv), _p(saf), _p(bgm),
                                              float(region_var), int(bool(revert_axis_swap)), b, frames, k, h, w, _p(rows), ld,
                                              _p(sparse), _stream(lib)), "lfdm_lfae_motion_inputs_f32")
    return rows, sparse


def lfae_motion_combine(heads, sparse, has_occ):
    """lfdm_lfae_motion_combine_f32: heads = channels-last rows (N*h*w, >= K+1 [+1]) of the mask (+ occlusion) convolutions ->
    (optical_flow (N, h, w, 2), occlusion_map (N, 1, h, w) or None)."""
    lib = _lib()
    _chk(lib, heads, sparse)
    n, k1, h, w, _ = sparse.shape
    flow = torch.empty(n, h, w, 2, dtype=torch.float32, device=sparse.device)
    occ = torch.empty(n, 1, h, w, dtype=torch.float32, device=sparse.device) if has_occ else None
    lib.check(lib.lfdm_lfae_motion_combine_f32(_p(heads), _ld(heads), _p(sparse), n, k1 - 1, h * w, _p(flow), _p(occ),
                                               _stream(lib)), "lfdm_lfae_motion_combine_f32")
    return flow, occ


def pack_wino_weight_grouped(ws):
    """[(Cout_g, Cin_g, 3, 3)] * G -> (G, 16, Cin_g/16, Cout_g, 16): the filters of a grouped 3x3 convolution
    (lfdm_conv_params.groups), each group's Winograd pack back to back."""
    packs = [pack_wino_weight(w.contiguous(), coutp=w.shape[0]) for w in ws]
    return torch.stack(packs).contiguous()


def pack_ln_conv_weight(w, gamma):
    """1x1 conv / linear weight (Cout, Cin[,1,1]) preceded by a channel LayerNorm with scale gamma (Cin,):
    returns (packed W' = W*gamma, ln_wsum (coutp,) = sum_c W'[o][c]) for lfdm_conv_params.ln_wsum."""
    w2 = w.reshape(w.shape[0], -1).float() * gamma.reshape(1, -1).float()
    packed = pack_conv_weight(w2)
    wsum = torch.zeros(packed.shape[1], dtype=torch.float32, device=w.device)
    wsum[: w2.shape[0]] = w2.double().sum(dim=1).float()
    return packed, wsum


def pack_wino_weight(w, coutp=None, dgrad=False, out=None):
    """(Cout, Cin, 3, 3) -> Winograd F(2x2,3x3) filters U = G g G^T as [16][K/16][coutp][16] (position, reduction-channel
    chunk, output channel, channel in chunk) - the operand order conv_wino.hip loads (lfdm_conv_params.weight_wino).
    dgrad=True: the filters of the data-gradient convolution dY -> dX (channel roles exchanged, taps flipped);
    `w` may be a slice w[:, lo:hi] of the input-channel axis (no copy).  out: an existing pack of this geometry to refill IN PLACE
    (its address may be held by a captured graph).  lfdm_pack_wino_weight_f32."""
    lib = _lib()
    if w.dim() == 5:
        w = w[:, :, 0]
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and w.dtype == torch.float32
    assert w.stride(3) == 1 and w.stride(2) == 3 and w.stride(1) == 9, "input-channel slices of a contiguous filter only"
    _chk(lib, w)
    k, n = (cout, cin) if dgrad else (cin, cout)
    assert k % 16 == 0
    coutp = coutp or (out.shape[2] if out is not None else (n + 31) // 32 * 32)
    if out is None:
        out = torch.empty(16, k // 16, coutp, 16, dtype=torch.float32, device=w.device)
    assert tuple(out.shape) == (16, k // 16, coutp, 16) and out.is_contiguous() and out.device == w.device
    lib.check(lib.lfdm_pack_wino_weight_f32(_p(w), w.stride(0), cout, cin, coutp, int(dgrad), _p(out), _stream(lib)),
              "lfdm_pack_wino_weight_f32")
    return out


def pack_wino_weight_bf16(w, coutp=None):
    """(Cout, Cin, 3, 3) -> the bf16 operands of the opt-in bf16 Winograd launch (conv2d_cl(weight_wino_bf16=...), lfdm_conv2d_cl_wino_bf16):
    a torch.bfloat16 tensor [16][Cin/16][coutp][16] (position, channel chunk, output channel, channel in chunk - plain order), each element
    the round-to-nearest-even bf16 of the value pack_wino_weight(w) holds.  lfdm_pack_wino_weight_bf16."""
    lib = _lib()
    if w.dim() == 5:
        w = w[:, :, 0]
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and w.dtype == torch.float32 and cin % 16 == 0
    assert w.stride(3) == 1 and w.stride(2) == 3 and w.stride(1) == 9, "input-channel slices of a contiguous filter only"
    _chk(lib, w)
    coutp = coutp or (cout + 31) // 32 * 32
    out = torch.empty(16, cin // 16, coutp, 16, dtype=torch.bfloat16, device=w.device)
    lib.check(lib.lfdm_pack_wino_weight_bf16(_p(w), w.stride(0), cout, cin, coutp, _p(out), _stream(lib)), "lfdm_pack_wino_weight_bf16")
    return out


def pack_wino_weight_grouped_bf16(ws):
    """pack_wino_weight_grouped in bf16: (G, 16, Cin_g/16, Cout_g, 16) bfloat16, each group's pack_wino_weight_bf16 back to back."""
    return torch.stack([pack_wino_weight_bf16(w.contiguous(), coutp=w.shape[0]) for w in ws]).contiguous()


_PACK_JOB_TABLES = {}


def pack_wino_weights_multi(jobs):
    """lfdm_pack_wino_weights_multi_f32: jobs = [(w view (Cout, Cin, 3, 3) or an input-channel slice of one, packed output tensor, dgrad)]
    - every filter re-packed into its EXISTING output tensor by one launch.  The device job table is cached per job list (pointers)."""
    import numpy as np
    lib = _lib()
    key, recs, block0 = [], [], 0
    for w, out, dgrad in jobs:
        cout, cin = w.shape[0], w.shape[1]
        k, n = (cout, cin) if dgrad else (cin, cout)
        coutp = out.shape[2]
        assert out.shape == (16, k // 16, coutp, 16) and out.is_contiguous() and w.stride(3) == 1 and w.stride(2) == 3 and w.stride(1) == 9
        _chk(lib, w, out)
        recs.append((w.data_ptr(), out.data_ptr(), w.stride(0), cout, cin, coutp, int(bool(dgrad)), block0))
        key.append(recs[-1][:7])
        block0 += (k // 4 * coutp + 255) // 256          # one thread per four reduction channels (conv_wino.hip pack_wino_item)
    key = (tuple(key), str(jobs[0][1].device))
    table = _PACK_JOB_TABLES.get(key)
    if table is None:
        if len(_PACK_JOB_TABLES) > 16:
            _PACK_JOB_TABLES.clear()
        dt = np.dtype([("w", "<u8"), ("out", "<u8"), ("ld_o", "<i4"), ("cout", "<i4"), ("cin", "<i4"), ("coutp", "<i4"), ("dgrad", "<i4"),
                       ("block0", "<i4")])
        arr = np.array(recs, dtype=dt)
        assert arr.dtype.itemsize == 40
        table = _PACK_JOB_TABLES[key] = torch.from_numpy(arr.view(np.uint8).copy()).to(jobs[0][1].device)
    lib.check(lib.lfdm_pack_wino_weights_multi_f32(C.c_void_p(table.data_ptr()), len(recs), block0, _stream(lib)), "lfdm_pack_wino_weights_multi_f32")


def pack_wino4_weight(w, coutp=None):
    """(Cout, Cin, 3, 3) -> Winograd F(4x4,3x3) filters U = G g G^T as [36][Cin/8][coutp][8] (lfdm_conv_params.weight_wino4, the
    batched-shape schedule of conv_wino4.hip).  lfdm_pack_wino4_weight_f32."""
    lib = _lib()
    if w.dim() == 5:
        w = w[:, :, 0]
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and w.dtype == torch.float32 and cin % 8 == 0
    assert w.stride(3) == 1 and w.stride(2) == 3 and w.stride(1) == 9, "input-channel slices of a contiguous filter only"
    _chk(lib, w)
    coutp = coutp or (cout + 31) // 32 * 32
    out = torch.empty(36, cin // 8, coutp, 8, dtype=torch.float32, device=w.device)
    lib.check(lib.lfdm_pack_wino4_weight_f32(_p(w), w.stride(0), cout, cin, coutp, _p(out), _stream(lib)), "lfdm_pack_wino4_weight_f32")
    return out


def pack_planar_in_weight(w):
    """(Cout, Cin, kh, kw) -> [kh*kw*Cin][Cout] (tap-major, then channel) for conv_planar_in_cl."""
    if w.dim() == 5:
        w = w[:, :, 0]
    cout, cin, kh, kw = w.shape
    return w.permute(2, 3, 1, 0).reshape(kh * kw * cin, cout).contiguous()


# ---------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------

def conv_params(src0, weight, cout, kh, kw, n_img, hi, wi, *, src1=None, bias=None, pad=None, stride=1,
                upsample=False, reflect=False, residual=None, act=ACT_NONE, out=None, hq=None, wq=None,
                ho=None, wo=None, out_scale=1, out_off=(0, 0), ksplit=0, ln_wsum=None, ln_eps=1e-5,
                tile_counters=None, weight_wino=None, deconv4=None, groups=1, pool2=False, weight_wino4=None, weight_pw=None, res_gn=None):
    """Fills an lfdm_conv_params struct (allocating `out` if needed); returns (params, out).
    ksplit=0 lets the library choose (conv_plan reports the choice)."""
    lib = _lib()
    _chk(lib, src0, src1, weight, bias, residual, out, ln_wsum)
    cin = src0.shape[1] + (src1.shape[1] if src1 is not None else 0)
    if groups > 1:      # grouped convolution: Winograd form only, `weight` is not read (lfdm_conv_params.groups)
        assert weight_wino is not None and src1 is None and weight is weight_wino
        coutp = cout
    elif weight is None:     # Winograd-only call (training re-packs filters every step: no direct-form pack); conv2d_cl verifies
        assert weight_wino is not None and deconv4 is None          # with lfdm_conv2d_schedule that the library agrees
        weight, coutp = weight_wino, weight_wino.shape[2]
    else:
        assert weight.shape[0] == (kh * kw * cin + 31) // 32 and weight.shape[2] == 32, (weight.shape, kh, kw, cin)
        coutp = weight.shape[1]
    pad_y, pad_x = (kh // 2, kw // 2) if pad is None else pad
    h_in = hi * 2 if upsample else hi
    w_in = wi * 2 if upsample else wi
    if hq is None:
        hq = (h_in + 2 * pad_y - kh) // stride + 1
        wq = (w_in + 2 * pad_x - kw) // stride + 1
    if ho is None:
        ho, wo = (hq // 2, wq // 2) if pool2 else (hq * out_scale, wq * out_scale)
    if out is None:
        out = torch.empty(n_img * ho * wo, cout, dtype=torch.float32, device=src0.device)
    p = ConvParams()
    p.src0, p.src1 = _p(src0), _p(src1)
    p.c0, p.c1 = src0.shape[1], (src1.shape[1] if src1 is not None else 0)
    p.ld0, p.ld1 = _ld(src0), (_ld(src1) if src1 is not None else 0)
    p.n_img, p.hi, p.wi, p.hq, p.wq = n_img, hi, wi, hq, wq
    p.stride, p.upsample, p.pad_mode = stride, int(upsample), int(reflect)
    p.kh, p.kw, p.pad_y, p.pad_x = kh, kw, pad_y, pad_x
    p.weight, p.cout, p.coutp, p.bias = _p(weight), cout, coutp, _p(bias)
    p.out, p.ldo, p.ho, p.wo = _p(out), _ld(out), ho, wo
    p.out_scale, p.out_off_y, p.out_off_x = out_scale, out_off[0], out_off[1]
    p.residual, p.ldr = _p(residual), (_ld(residual) if residual is not None else 0)
    p.act, p.ksplit, p.partial = act, ksplit, None
    p.gn_partial, p.gn_groups, p.gn_pixels = None, 0, 0
    p.ln_wsum, p.ln_eps = _p(ln_wsum), ln_eps
    p.tile_counters, p.tile_counters_len = None, 0
    if tile_counters is not None:       # zero-initialised int32 words: split-K slabs are reduced inside the launch
        assert tile_counters.dtype == torch.int32 and tile_counters.is_contiguous()
        _chk(lib, tile_counters)
        p.tile_counters, p.tile_counters_len = tile_counters.data_ptr(), tile_counters.numel()
    p.weight_wino = None
    p.groups = groups if groups > 1 else 0
    if weight_wino is not None:
        _chk(lib, weight_wino)
        want = (16, cin // 16, coutp, 16) if groups <= 1 else (groups, 16, cin // groups // 16, coutp // groups, 16)
        assert kh == 3 and kw == 3 and weight_wino.shape == want and weight_wino.is_contiguous(), (weight_wino.shape, want)
        p.weight_wino = weight_wino.data_ptr()
    p.deconv4 = 0
    if deconv4 is not None:     # the four parity packs of pack_deconv_weight, stacked: ONE launch (lfdm_conv_params.deconv4)
        _chk(lib, deconv4)
        assert kh == 2 and kw == 2 and out_scale == 2 and deconv4.is_contiguous() and deconv4.shape == (4,) + tuple(weight.shape) \
            and deconv4.data_ptr() == weight.data_ptr(), "weight must be deconv4[0]"
        p.deconv4 = 1
    p.weight_wino4 = None
    if weight_wino4 is not None:        # F(4x4,3x3) form for batched shapes (the library decides: lfdm_conv2d_schedule == 4)
        _chk(lib, weight_wino4)
        assert weight_wino is not None and weight_wino4.shape == (36, cin // 8, coutp, 8) and weight_wino4.is_contiguous()
        p.weight_wino4 = weight_wino4.data_ptr()
    p.weight_pw = None
    if weight_pw is not None:          # the same 1x1 filter in operand order for the pointwise schedule (pack_pw_weight)
        _chk(lib, weight_pw)
        assert weight_pw.numel() == weight.numel() and weight_pw.is_contiguous()      # (1x1, or the gather form of the 4x4 / stride-2 Downsample)
        p.weight_pw = weight_pw.data_ptr()
    keep_gn = (weight_pw,)
    p.gn_in_partial, p.defer_reduce = None, 0      # (reserved since ABI 12: must stay NULL / 0)
    # res_gn = dict(partial, nchunk, pixels, gamma, beta, groups=8, eps=1e-5): `residual` is a RAW convolution output whose GroupNorm + SiLU is
    # applied in this (pointwise) convolution's epilogue (lfdm_conv_params.res_gn_*)
    p.res_gn_partial = None
    if res_gn is not None:
        gp, gg, gb = res_gn["partial"], res_gn["gamma"], res_gn["beta"]
        _chk(lib, gp, gg, gb)
        assert residual is not None and gg.numel() == cout == gb.numel() and gp.is_contiguous()
        p.res_gn_partial, p.res_gn_nchunk, p.res_gn_groups, p.res_gn_pixels = _p(gp), int(res_gn["nchunk"]), int(res_gn.get("groups", 8)), int(res_gn["pixels"])
        p.res_gn_gamma, p.res_gn_beta, p.res_gn_eps = _p(gg), _p(gb), float(res_gn.get("eps", 1e-5))
        keep_gn = keep_gn + (gp, gg, gb)
    p.pool2 = int(bool(pool2))          # Winograd schedule only (the library refuses it elsewhere): the 2x2 average pool behind conv -> act
    p._keep = (src0, src1, weight, bias, residual, out, ln_wsum, tile_counters, weight_wino, deconv4, weight_wino4) + keep_gn   # keep the tensors alive with the struct
    return p, out


def conv_partial_floats(p):
    """Split-K scratch the library wants for these params (slabs [+ LayerNorm row statistics]), in floats."""
    return _lib().lfdm_conv2d_partial_bytes(C.byref(p)) // 4


def conv_plan_slabs(p):
    """Slabs per output tile the launch will sum (lfdm_conv2d_plan_slabs): ksplit, or more for a balanced Winograd launch."""
    return _lib().lfdm_conv2d_plan_slabs(C.byref(p))


class WinogradUnavailable(RuntimeError):
    pass


def conv_plan(p):
    """(tile_rows, ksplit) the library will use for these params (lfdm_conv2d_plan)."""
    lib = _lib()
    rows, ks = C.c_int(0), C.c_int(0)
    lib.check(lib.lfdm_conv2d_plan(C.byref(p), C.byref(rows), C.byref(ks)), "lfdm_conv2d_plan")
    return rows.value, ks.value


def conv_schedule(p):
    """lfdm_conv2d_schedule: 0 = implicit GEMM, 1 = K-split across waves, 2 = Winograd F(2x2), 3 = pointwise, 4 = Winograd F(4x4)."""
    return _lib().lfdm_conv2d_schedule(C.byref(p))


def conv_launch(p):
    lib = _lib()
    lib.check(lib.lfdm_conv2d_cl_f32(C.byref(p), _stream(lib)), "lfdm_conv2d_cl_f32")


def _chk_wino_bf16(lib, p, wwb):
    """The bf16 pack that goes with the fp32 Winograd pack of `p` (same filter, same shape)."""
    if wwb.dtype != torch.bfloat16 or not wwb.is_contiguous():
        raise TypeError("weight_wino_bf16: a contiguous torch.bfloat16 pack (pack_wino_weight_bf16) expected, got %s" % wwb.dtype)
    if (lib.kind == "hip") != wwb.is_cuda:
        raise RuntimeError("weight_wino_bf16 must live where the library runs (GPU for hip, CPU for emu)")
    ww = p._keep[8]
    if ww is None or tuple(wwb.shape) != tuple(ww.shape):
        raise ValueError("weight_wino_bf16 needs weight_wino (the fp32 pack that decides the plan) of the same shape")


def conv_launch_wino_bf16(p, weight_wino_bf16):
    """lfdm_conv2d_cl_wino_bf16: the launch conv_launch(p) would run, on bf16 operands (the library refuses geometries that are not on the
    Winograd F(2x2) schedule)."""
    lib = _lib()
    _chk_wino_bf16(lib, p, weight_wino_bf16)
    lib.check(lib.lfdm_conv2d_cl_wino_bf16(C.byref(p), _p(weight_wino_bf16), _stream(lib)), "lfdm_conv2d_cl_wino_bf16")


def conv2d_cl(src0, weight, cout, kh, kw, n_img, hi, wi, *, partial=None, gn_partial=None, gn_groups=8,
              gn_pixels=0, weight_wino_bf16=None, **kw_):
    """One convolution (see conv_params for the keywords).  Split-K scratch is allocated on demand.
    weight_wino_bf16 (with weight_wino): the Winograd F(2x2) launch on bf16 operands (pack_wino_weight_bf16 of the same filter) - only where
    the library picks that schedule for these parameters (WinogradUnavailable otherwise)."""
    lib = _lib()
    _chk(lib, partial, gn_partial)
    p, out = conv_params(src0, weight, cout, kh, kw, n_img, hi, wi, **kw_)
    if weight_wino_bf16 is not None:
        _chk_wino_bf16(lib, p, weight_wino_bf16)
        if kw_.get("pool2") or lib.lfdm_conv2d_schedule(C.byref(p)) != 2:
            raise WinogradUnavailable("bf16 operands exist on the Winograd F(2x2,3x3) schedule only, without pool2: the library would not run it "
                                      "for this geometry")
    if (weight is None or kw_.get("pool2")) and lib.lfdm_conv2d_schedule(C.byref(p)) not in ((2,) if kw_.get("pool2") else (2, 4)):
        raise WinogradUnavailable("the library would not run the Winograd schedule for this geometry: pass the direct-form pack / "
                                  "run the pooling as a launch of its own")
    if gn_partial is not None:      # before the plan is asked for: the pointwise schedule has no fused statistics
        p.gn_partial, p.gn_groups, p.gn_pixels = _p(gn_partial), gn_groups, gn_pixels
    need = conv_partial_floats(p)          # (also non-zero for a ksplit = 1 plan that balances its Winograd launch: lfdm_hip.h, tile_counters)
    if need > 0:
        if partial is None or partial.numel() < need:
            partial = torch.empty(need, dtype=torch.float32, device=src0.device)
        p.partial = _p(partial)
    if weight_wino_bf16 is not None:
        conv_launch_wino_bf16(p, weight_wino_bf16)
    else:
        conv_launch(p)
    return out


def pack_smalln_weight(w, bias=None):
    """(Cout <= 4, Cin, k, k) -> ([k*k][Cin][4] filters innermost, zero padded; bias padded to 4)."""
    cout, cin, kh, kw = w.shape
    assert cout <= 4 and kh == kw
    wp = torch.zeros(kh * kw, cin, 4, dtype=torch.float32, device=w.device)
    wp[:, :, :cout] = w.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    bp = torch.zeros(4, dtype=torch.float32, device=w.device)
    if bias is not None:
        bp[:cout] = bias
    return wp.contiguous(), bp


def conv2d_smalln_cl(x, wpacked, bias4, cout, k, n_img, h, w, *, act=ACT_NONE, out=None):
    """Convolution with <= 4 output channels (4x4x1 MFMA blocks); out rows have stride out.stride(0) >= cout."""
    lib = _lib()
    _chk(lib, x, wpacked, bias4, out)
    if out is None:
        out = torch.empty(n_img * h * w, 4, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_conv2d_smalln_cl_f32(_p(x), _ld(x), x.shape[1], n_img, h, w, _p(wpacked), _p(bias4), _p(out),
                                            _ld(out), cout, k, act, _stream(lib)), "lfdm_conv2d_smalln_cl_f32")
    return out


def deconv4x4s2_cl(src, packs, cout, n_img, hi, wi, *, bias=None, out=None):
    """ConvTranspose (1,4,4) stride (1,2,2) pad (0,1,1) as four parity 2x2 convolutions: ONE launch when `packs` is the
    stacked tensor of pack_deconv4_weight, four launches for the list of pack_deconv_weight."""
    if out is None:
        out = torch.empty(n_img * 4 * hi * wi, cout, dtype=torch.float32, device=src.device)
    if torch.is_tensor(packs):
        conv2d_cl(src, packs[0], cout, 2, 2, n_img, hi, wi, bias=bias, pad=(1, 1), out=out, hq=hi, wq=wi, ho=2 * hi, wo=2 * wi,
                  out_scale=2, deconv4=packs)
        return out
    for py, px, w in packs:
        conv2d_cl(src, w, cout, 2, 2, n_img, hi, wi, bias=bias, pad=(1 - py, 1 - px), out=out,
                  hq=hi, wq=wi, ho=2 * hi, wo=2 * wi, out_scale=2, out_off=(py, px))
    return out


def groupnorm_silu_cl(x, batch, gamma, beta, *, groups=8, scale_shift=None, residual=None, eps=1e-5,
                      silu=True, out=None, ws=None):
    lib = _lib()
    rows, ch = x.shape
    pixels = rows // batch
    _chk(lib, x, gamma, beta, scale_shift, residual, out, ws)
    _dense(x, residual, out)
    if out is None:
        out = torch.empty_like(x)
    need = lib.lfdm_groupnorm_ws_bytes(batch, pixels, ch)
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_groupnorm_silu_cl_f32(_p(x), _p(out), batch, pixels, ch, groups, _p(gamma),
                                             _p(beta), _p(scale_shift),
                                             _ld(scale_shift) if scale_shift is not None else 0,
                                             _p(residual), eps, int(silu), _p(ws),
                                             ws.numel() * 4, _stream(lib)), "lfdm_groupnorm_silu_cl_f32")
    return out


def groupnorm_apply_cl(x, batch, gamma, beta, partial, nchunk, *, groups=8, scale_shift=None, residual=None,
                       eps=1e-5, silu=True, out=None, ws=None):
    """GroupNorm whose statistics came from the producing convolution (gn_partial)."""
    lib = _lib()
    rows, ch = x.shape
    _chk(lib, x, gamma, beta, partial, scale_shift, residual, out, ws)
    _dense(x, residual, out, partial)
    if out is None:
        out = torch.empty_like(x)
    if ws is None:
        ws = torch.empty(batch * 2 * ch, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_groupnorm_apply_cl_f32(_p(x), _p(out), batch, rows // batch, ch, groups, _p(gamma), _p(beta),
                                              _p(scale_shift),
                                              _ld(scale_shift) if scale_shift is not None else 0,
                                              _p(residual), eps, int(silu), _p(partial), nchunk, _p(ws),
                                              ws.numel() * 4, _stream(lib)), "lfdm_groupnorm_apply_cl_f32")
    return out


def layernorm_cl(x, gamma, eps=1e-5, out=None):
    lib = _lib()
    _chk(lib, x, gamma, out)
    _dense(x, out)
    if out is None:
        out = torch.empty_like(x)
    lib.check(lib.lfdm_layernorm_cl_f32(_p(x), _p(out), x.shape[0], x.shape[1], _p(gamma), eps,
                                        _stream(lib)), "lfdm_layernorm_cl_f32")
    return out


def attention_cl(qkv, batch, frames, hw, mode, *, bias=None, rot_cos=None, rot_sin=None, out=None):
    lib = _lib()
    _chk(lib, qkv, bias, rot_cos, rot_sin, out)
    assert qkv.shape[1] == 768 and qkv.is_contiguous()
    if out is None:
        out = torch.empty(qkv.shape[0], 256, dtype=torch.float32, device=qkv.device)
    lib.check(lib.lfdm_attention_cl_f32(_p(qkv), _p(out), batch, frames, hw, mode, _p(bias),
                                        _p(rot_cos), _p(rot_sin), _stream(lib)), "lfdm_attention_cl_f32")
    return out


ATTN_SHORT_MAX = 64       # tokens per sequence of attention_cl and the fused forms
ATTN_LONG_MAX = 256       # tokens per sequence of attention_long_cl


def attention_long_cl(qkv, batch, frames, hw, mode, *, bias=None, rot_cos=None, rot_sin=None, out=None, stats=None):
    """attention_cl over 65 .. 256 tokens per sequence (streaming kernel; 64 and fewer are refused: attention_cl owns them).
    stats: optional (nseq * 8, 2, L) tensor that receives the row maxima and row sums."""
    lib = _lib()
    _chk(lib, qkv, bias, rot_cos, rot_sin, out, stats)
    assert qkv.shape[1] == 768 and qkv.is_contiguous()
    if stats is not None:
        seq = frames if mode == 0 else hw
        nseq = batch * hw if mode == 0 else batch * frames
        assert stats.is_contiguous() and stats.numel() == nseq * 8 * 2 * seq
    if out is None:
        out = torch.empty(qkv.shape[0], 256, dtype=torch.float32, device=qkv.device)
    lib.check(lib.lfdm_attention_long_cl_f32(_p(qkv), _p(out), batch, frames, hw, mode, _p(bias),
                                             _p(rot_cos), _p(rot_sin), _p(stats), _stream(lib)), "lfdm_attention_long_cl_f32")
    return out


def temporal_attention_fused_cl(x, wqkv, batch, frames, hw, *, bias=None, rot_cos=None, rot_sin=None, eps=1e-5, out=None):
    """LayerNorm + to_qkv + temporal attention in one launch (C in {64, 128}); wqkv (768, C) with gamma folded."""
    lib = _lib()
    _chk(lib, x, wqkv, bias, rot_cos, rot_sin, out)
    c = x.shape[1]
    assert wqkv.shape == (768, c) and wqkv.is_contiguous()
    if out is None:
        out = torch.empty(x.shape[0], 256, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_temporal_attention_fused_cl_f32(_p(x), _ld(x), c, _p(wqkv), _p(out), batch, frames, hw, _p(bias),
                                                       _p(rot_cos), _p(rot_sin), eps, _stream(lib)),
              "lfdm_temporal_attention_fused_cl_f32")
    return out


def pack_pw_weight(packed):
    """Direct-form pack of a 1x1 filter ([K/32][coutp][32], pack_conv_weight) -> the MFMA-operand order of the pointwise schedule
    (lfdm_conv_params.weight_pw): [K/32][coutp/32][4 u][64 lanes = 32*kh + column][4 e], k % 32 = 8u + 4kh + e."""
    g, coutp, k32 = packed.shape
    assert k32 == 32 and coutp % 32 == 0
    # (g, ct, column, u, kh, e) -> (g, ct, u, kh, column, e)
    return packed.reshape(g, coutp // 32, 32, 4, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous().view(g, coutp // 32, 4, 64, 4)


def pack_tattn_weights(wqkv_folded, wout):
    """(768, 64) LayerNorm-folded to_qkv weight and (64, 256) to_out weight -> the MFMA-operand order of
    lfdm_temporal_attention_fused_out_cl_f32 (every fragment load = one contiguous 1 KB): ([3][8][2][4][64][4], [4][16][64][4])."""
    assert wqkv_folded.shape == (768, 64) and wout.shape == (64, 256)
    # rows: which(3) head(8) half(2) l15(16); columns: lq(4) quad(4) e(4)  ->  which head half quad (lq l15) e
    wq = wqkv_folded.float().reshape(3, 8, 2, 16, 4, 4, 4).permute(0, 1, 2, 5, 4, 3, 6).contiguous().view(3, 8, 2, 4, 64, 4)
    # rows: ct(4) l15(16); columns: S(16) lq(4) e(4)  ->  ct S (lq l15) e
    wo = wout.float().reshape(4, 16, 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(4, 16, 64, 4)
    return wq, wo


def temporal_attention_fused_out_cl(x, wqkv, wout, batch, frames, hw, *, bias=None, rot_cos=None, rot_sin=None, eps=1e-5, out=None):
    """The whole temporal-attention block in one launch (C == 64): out = x + to_out(attention(LayerNorm(x))); wqkv, wout =
    pack_tattn_weights(W_qkv * gamma, W_out)."""
    lib = _lib()
    _chk(lib, x, wqkv, wout, bias, rot_cos, rot_sin, out)
    c = x.shape[1]
    assert c == 64 and wqkv.shape == (3, 8, 2, 4, 64, 4) and wqkv.is_contiguous() and wout.shape == (4, 16, 64, 4) and wout.is_contiguous()
    if out is None:
        out = torch.empty(x.shape[0], c, dtype=torch.float32, device=x.device)
    assert out.data_ptr() != x.data_ptr()
    lib.check(lib.lfdm_temporal_attention_fused_out_cl_f32(_p(x), _ld(x), c, _p(wqkv), _p(wout), _p(out), _ld(out), batch, frames, hw,
                                                           _p(bias), _p(rot_cos), _p(rot_sin), eps, _stream(lib)),
              "lfdm_temporal_attention_fused_out_cl_f32")
    return out


def pack_linattn_weights(wqkv_folded):
    """(768, 64) LayerNorm-folded to_qkv weight of SpatialLinearAttention -> the MFMA-operand order of lfdm_linear_attention_fused_cl_f32:
    [3 = q|k|v][8 heads][8 quads][64 lanes = 32*kh + l31][4]  <-  W[which*256 + head*32 + l31][32*kh + 4*quad + e]."""
    assert wqkv_folded.shape == (768, 64)
    # rows: which(3) head(8) l31(32); columns: kh(2) quad(8) e(4)  ->  which head quad (kh l31) e
    return wqkv_folded.float().reshape(3, 8, 32, 2, 8, 4).permute(0, 1, 4, 3, 2, 5).contiguous().view(3, 8, 8, 64, 4)


def linear_attention_fused_ws_floats(n_frames, hw):
    return (int(_lib().lfdm_linear_attention_fused_ws_bytes(n_frames, hw)) + 3) // 4


def linear_attention_fused_cl(x, wqkv, n_frames, hw, *, eps=1e-5, out=None, ws=None):
    """LayerNorm + to_qkv + linear attention core without materialising qkv (C == 64); wqkv = pack_linattn_weights(W_qkv * gamma)."""
    lib = _lib()
    _chk(lib, x, wqkv, out, ws)
    assert x.shape[1] == 64 and wqkv.shape == (3, 8, 8, 64, 4) and wqkv.is_contiguous()
    if out is None:
        out = torch.empty(x.shape[0], 256, dtype=torch.float32, device=x.device)
    need = lib.lfdm_linear_attention_fused_ws_bytes(n_frames, hw)
    if ws is not None:
        ws = ws.reshape(-1)
    if ws is None or ws.numel() * 4 < need:
        ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_linear_attention_fused_cl_f32(_p(x), _ld(x), x.shape[1], _p(wqkv), _p(out), n_frames, hw, eps,
                                                     _p(ws), ws.numel() * 4, _stream(lib)),
              "lfdm_linear_attention_fused_cl_f32")
    return out


def pack_linattn_out_weight(wout):
    """(64, 256) to_out weight of SpatialLinearAttention -> the MFMA-operand order of lfdm_linear_attention_fused_out_cl_f32:
    [8 heads][2 row blocks][4 quads][64 lanes = 32*kh + c_local][4]  <-  Wout[32*cb + c_local][32*h + 8*quad + 4*kh + e]."""
    w = wout.float().reshape(64, 256)
    # rows: cb(2) c_local(32); columns: h(8) quad(4) kh(2) e(4)  ->  h cb quad (kh c_local) e
    return w.reshape(2, 32, 8, 4, 2, 4).permute(2, 0, 3, 4, 1, 5).contiguous().view(8, 2, 4, 64, 4)


def linear_attention_fused_out_cl(x, wqkv, wout, bias_out, n_frames, hw, *, eps=1e-5, out=None, ws=None):
    """The whole Residual(PreNorm(SpatialLinearAttention)) block at C == 64: out = x + to_out(linear_attention(LayerNorm(x))) + bias;
    wqkv = pack_linattn_weights(W_qkv * gamma), wout = pack_linattn_out_weight(W_out)."""
    lib = _lib()
    _chk(lib, x, wqkv, wout, bias_out, out, ws)
    assert x.shape[1] == 64 and wqkv.shape == (3, 8, 8, 64, 4) and wqkv.is_contiguous() and wout.shape == (8, 2, 4, 64, 4) and wout.is_contiguous()
    if out is None:
        out = torch.empty(x.shape[0], 64, dtype=torch.float32, device=x.device)
    assert out.data_ptr() != x.data_ptr()
    need = lib.lfdm_linear_attention_fused_ws_bytes(n_frames, hw)
    if ws is not None:
        ws = ws.reshape(-1)
    if ws is None or ws.numel() * 4 < need:
        ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_linear_attention_fused_out_cl_f32(_p(x), _ld(x), x.shape[1], _p(wqkv), _p(wout), _p(bias_out), _p(out), _ld(out),
                                                         n_frames, hw, eps, _p(ws), ws.numel() * 4, _stream(lib)),
              "lfdm_linear_attention_fused_out_cl_f32")
    return out


def linear_attention_lowres_cl(x, wqkv, wsum, n_frames, hw, *, eps=1e-5, out=None):
    """LayerNorm + to_qkv + linear attention core in ONE launch (low-resolution levels: hw <= 64 or 192 < hw <= 256 pixels per frame,
    C % 64 == 0); wqkv (768, C) with gamma folded, wsum (768,) = its row sums (pack_ln_conv_weight)."""
    lib = _lib()
    _chk(lib, x, wqkv, wsum, out)
    assert wqkv.shape == (768, x.shape[1]) and wqkv.is_contiguous() and wsum.numel() >= 768
    if out is None:
        out = torch.empty(x.shape[0], 256, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_linear_attention_lowres_cl_f32(_p(x), _ld(x), x.shape[1], _p(wqkv), _p(wsum), _p(out), n_frames, hw, eps,
                                                      _stream(lib)), "lfdm_linear_attention_lowres_cl_f32")
    return out


def linear_attention_lowres_ok(hw, channels):
    return channels % 64 == 0 and (hw <= 64 or 192 < hw <= 256)


def attention_lowres_cl(x, wqkv, wsum, batch, frames, hw, mode, *, bias=None, rot_cos=None, rot_sin=None, eps=1e-5, out=None):
    """LayerNorm + to_qkv + softmax attention core in ONE launch (<= 64 tokens per sequence, C % 64 == 0): mode 0 over the frames of
    a pixel (rotary tables + relative-position bias), mode 1 over the pixels of a frame."""
    lib = _lib()
    _chk(lib, x, wqkv, wsum, bias, rot_cos, rot_sin, out)
    assert wqkv.shape == (768, x.shape[1]) and wqkv.is_contiguous() and wsum.numel() >= 768
    if out is None:
        out = torch.empty(x.shape[0], 256, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_attention_lowres_cl_f32(_p(x), _ld(x), x.shape[1], _p(wqkv), _p(wsum), _p(out), batch, frames, hw, mode,
                                               _p(bias), _p(rot_cos), _p(rot_sin), eps, _stream(lib)), "lfdm_attention_lowres_cl_f32")
    return out


def linear_attention_cl(qkv, n_frames, hw, *, out=None, ws=None):
    lib = _lib()
    _chk(lib, qkv, out, ws)
    assert qkv.shape[1] == 768 and qkv.is_contiguous()
    if out is None:
        out = torch.empty(qkv.shape[0], 256, dtype=torch.float32, device=qkv.device)
    need = lib.lfdm_linear_attention_ws_bytes(n_frames)
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.float32, device=qkv.device)
    lib.check(lib.lfdm_linear_attention_cl_f32(_p(qkv), _p(out), n_frames, hw, _p(ws), ws.numel() * 4,
                                               _stream(lib)), "lfdm_linear_attention_cl_f32")
    return out


def linear_small(x, w, bias=None, *, act_in=ACT_NONE, act_out=ACT_NONE, out=None):
    lib = _lib()
    _chk(lib, x, w, bias, out)
    batch, k = x.shape
    n = w.shape[0]
    assert w.shape[1] == k and w.stride(1) == 1
    if out is None:
        out = torch.empty(batch, n, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_linear_small_f32(_p(x), _p(w), _p(bias), _p(out), batch, k, n, _ld(x),
                                        w.stride(0), out.stride(0), act_in, act_out, _stream(lib)),
              "lfdm_linear_small_f32")
    return out


def step_cond(step_table, batch_base, step_dev, out):
    lib = _lib()
    _chk(lib, step_table, batch_base, step_dev, out)
    batch, n = batch_base.shape
    lib.check(lib.lfdm_step_cond_f32(_p(step_table), _p(batch_base), _p(step_dev), _p(out), batch, n,
                                     _stream(lib)), "lfdm_step_cond_f32")
    return out


def calib_mfma(device, blocks=256, iters=4000, reps=3):
    """Box calibration (lfdm_calib_mfma_f32; never on the product path): the fp32 matrix rate and the shader clock this GPU holds
    under a pure v_mfma_f32_32x32x2_f32 load RIGHT NOW.  Returns {"tflops", "mhz", "mhz_min", "mhz_max", "us"} (best of `reps`)."""
    lib = _lib()
    out = torch.zeros(2 * blocks + 256, dtype=torch.float32, device=device)
    _chk(lib, out)
    launch = lambda n: lib.check(lib.lfdm_calib_mfma_f32(_p(out), blocks, n, _stream(lib)), "lfdm_calib_mfma_f32")
    launch(64)
    # an idle chip sits at ~500 MHz and needs some milliseconds of load to ramp: 30 ms of the same kernel first (round 4, call A: the
    # un-warmed figure read 134 TFLOP/s at 2115 MHz on a box that holds 2390 MHz)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(60):
        launch(iters)
    e1.record()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(iters)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3
        v = out[:2 * blocks].view(blocks, 2).double().cpu()
        mhz = 100.0 * v[:, 0] / v[:, 1].clamp(min=1.0)
        row = {"tflops": round(blocks * 4 * iters * 4 * 4096.0 / us / 1e6, 1), "mhz": round(float(mhz.median()), 0),
               "mhz_min": round(float(mhz.min()), 0), "mhz_max": round(float(mhz.max()), 0), "us": round(us, 1)}
        if best is None or row["tflops"] > best["tflops"]:
            best = row
    return best


def sinusoidal_freqs(dim, device):
    """fp32 frequency table, computed with the reference's expression (video_flow_diffusion.py:148-150)."""
    import math
    half = dim // 2
    return torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1))).to(device)


def sinusoidal(t_dev, freqs, batch, dim, *, t_stride=1, out=None):
    lib = _lib()
    _chk(lib, t_dev, freqs, out)
    assert t_dev.dtype == torch.int32
    if out is None:
        out = torch.empty(batch, dim, dtype=torch.float32, device=t_dev.device)
    lib.check(lib.lfdm_sinusoidal_f32(_p(t_dev), t_stride, _p(freqs), _p(out), batch, dim, _ld(out),
                                      _stream(lib)), "lfdm_sinusoidal_f32")
    return out


def conv_planar_in_cl(x, batch, cin, cin_total, frames, h, w, wgt, kh, kw, cout, *, bias=None,
                      add_term=None, act=ACT_NONE, out=None):
    lib = _lib()
    _chk(lib, x, wgt, bias, add_term, out)
    if out is None:
        out = torch.empty(batch * frames * h * w, cout, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_conv_planar_in_cl_f32(_p(x), batch, cin, cin_total, frames, h, w, _p(wgt), kh, kw,
                                             cout, _p(bias), _p(add_term), _p(out), _ld(out), act,
                                             _stream(lib)), "lfdm_conv_planar_in_cl_f32")
    return out


def heads_cl_to_planar(y_flow, y_occ, w_flow, b_flow, w_occ, b_occ, batch, frames, hw, *, out=None):
    """y_flow / y_occ: (rows, C) each, equal row stride (column slices of one (rows, 2C) tensor are fine)."""
    lib = _lib()
    _chk(lib, y_flow, y_occ, w_flow, b_flow, w_occ, b_occ, out)
    ch = y_flow.shape[1]
    assert y_flow.stride(0) == y_occ.stride(0) and y_flow.stride(1) == 1 and y_occ.stride(1) == 1
    if out is None:
        out = torch.empty(batch, 3, frames, hw, dtype=torch.float32, device=y_flow.device)
    lib.check(lib.lfdm_heads_cl_to_planar_f32(_p(y_flow), _p(y_occ), ch, _ld(y_flow), _p(w_flow), _p(b_flow),
                                              _p(w_occ), _p(b_occ), _p(out), batch, frames, hw,
                                              _stream(lib)), "lfdm_heads_cl_to_planar_f32")
    return out


def heads_res_cl_to_planar(y_flow, y_occ, w_flow, b_flow, w_occ, b_occ, x0, x1, w_extra, batch, frames, hw, *, out=None):
    """heads_cl_to_planar with the ResnetBlocks' res_conv(cat(x0, x1)) folded in: w_extra (3, c0 + c1) = [W_flow Wres_flow ; W_occ Wres_occ],
    b_flow / b_occ include W1 bres (lfdm_heads_res_cl_to_planar_f32)."""
    lib = _lib()
    _chk(lib, y_flow, y_occ, w_flow, b_flow, w_occ, b_occ, x0, x1, w_extra, out)
    ch = y_flow.shape[1]
    c0, c1 = x0.shape[1], (x1.shape[1] if x1 is not None else 0)
    assert y_flow.stride(0) == y_occ.stride(0) and y_flow.stride(1) == 1 and y_occ.stride(1) == 1
    assert w_extra.shape == (3, c0 + c1) and w_extra.is_contiguous() and x0.stride(1) == 1
    if out is None:
        out = torch.empty(batch, 3, frames, hw, dtype=torch.float32, device=y_flow.device)
    lib.check(lib.lfdm_heads_res_cl_to_planar_f32(_p(y_flow), _p(y_occ), ch, _ld(y_flow), _p(w_flow), _p(b_flow), _p(w_occ), _p(b_occ),
                                                  _p(x0), _ld(x0), c0, _p(x1), _ld(x1) if x1 is not None else 0, c1, _p(w_extra),
                                                  _p(out), batch, frames, hw, _stream(lib)), "lfdm_heads_res_cl_to_planar_f32")
    return out


def heads_gn_res_cl_to_planar(y, partial, nchunk, gamma, beta, w_flow, b_flow, w_occ, b_occ, x0, x1, w_extra, batch, frames, hw, *, groups=16,
                              eps=1e-5, out=None):
    """heads_res_cl_to_planar with the preceding GroupNorm + SiLU folded in: y (rows, 2C) = the RAW second convolution of the merged heads block,
    partial / nchunk = its fused statistics, gamma / beta (2C,) (lfdm_heads_gn_res_cl_to_planar_f32)."""
    lib = _lib()
    _chk(lib, y, partial, gamma, beta, w_flow, b_flow, w_occ, b_occ, x0, x1, w_extra, out)
    ch = y.shape[1] // 2
    c0, c1 = x0.shape[1], (x1.shape[1] if x1 is not None else 0)
    _ld(y)
    assert y.stride(1) == 1 and y.shape[1] == 2 * ch and gamma.numel() == 2 * ch == beta.numel() and partial.is_contiguous()
    assert w_extra.shape == (3, c0 + c1) and w_extra.is_contiguous() and x0.stride(1) == 1 and w_flow.numel() == 2 * ch and w_occ.numel() == ch
    if out is None:
        out = torch.empty(batch, 3, frames, hw, dtype=torch.float32, device=y.device)
    lib.check(lib.lfdm_heads_gn_res_cl_to_planar_f32(_p(y), _ld(y), ch, _p(partial), nchunk, groups, _p(gamma), _p(beta), eps, _p(w_flow), _p(b_flow),
                                                     _p(w_occ), _p(b_occ), _p(x0), _ld(x0), c0, _p(x1), _ld(x1) if x1 is not None else 0, c1,
                                                     _p(w_extra), _p(out), batch, frames, hw, _stream(lib)), "lfdm_heads_gn_res_cl_to_planar_f32")
    return out


def sampler_ws(batch, n, device):
    """Workspace of sampler_step / abs_quantile, initialised (lfdm_sampler_ws_init: histograms + end-of-step ticket cleared)."""
    lib = _lib()
    ws = torch.empty((lib.lfdm_sampler_ws_bytes(batch, n) + 3) // 4, dtype=torch.float32, device=device)
    _chk(lib, ws)
    lib.check(lib.lfdm_sampler_ws_init(_p(ws), ws.numel() * 4, batch, n, _stream(lib)), "lfdm_sampler_ws_init")
    return ws


def _known_operands(what, x, known, known_noise, frame_mask, level, frames, elem_mask, need_level=True):
    """The known operands of sampler_step / sampler_step_ms / known_blend / known_blend_elem as the filled _native.KnownOperands (zeroed: no
    conditioning): all of them or none, in ONE of the two forms - frame_mask (B, frames) with frames, or elem_mask of x's shape (one byte per
    element); both masks are bool or uint8, used as bytes."""
    k = _native.KnownOperands()
    elem = elem_mask is not None
    if elem and (frame_mask is not None or frames is not None):
        raise ValueError("%s: elem_mask and frame_mask / frames exclude each other" % what)
    operands = dict(known=known, known_noise=known_noise, **(dict(elem_mask=elem_mask) if elem else dict(frame_mask=frame_mask, frames=frames)))
    if need_level:
        operands["level"] = level
    if all(v is None for v in operands.values()):
        return k
    if any(v is None for v in operands.values()):
        raise ValueError("%s: %s go together (all of them or none)" % (what, ", ".join(operands)))
    batch = x.shape[0]
    n = x.numel() // batch
    for name, t in (("known", known), ("known_noise", known_noise)):
        if t.dtype != torch.float32 or t.numel() != x.numel() or not t.is_contiguous() or t.device != x.device:
            raise ValueError("%s: %s must be a contiguous float32 tensor of x's %d elements on x's device" % (what, name, x.numel()))
    if need_level and (level.dtype != torch.float32 or level.dim() != 2 or level.shape[1] != 2 or not level.is_contiguous()
                       or level.device != x.device):
        raise ValueError("%s: level must be a contiguous (steps + 1, 2) float32 tensor on x's device" % what)
    mask = elem_mask if elem else frame_mask
    if mask.dtype not in (torch.bool, torch.uint8) or not mask.is_contiguous() or mask.device != x.device:
        raise ValueError("%s: the mask must be a contiguous bool / uint8 tensor on x's device" % what)
    if elem:
        if tuple(elem_mask.shape) != tuple(x.shape):
            raise ValueError("%s: elem_mask must have x's shape %s, got %s" % (what, tuple(x.shape), tuple(elem_mask.shape)))
        k.elem_mask = _p(elem_mask)
    else:
        frames = int(frames)
        if frames < 1 or n % frames != 0:
            raise ValueError("%s: frames = %d does not divide the sample's %d elements" % (what, frames, n))
        if x.dim() >= 4:                                     # planar (B, C, T, ...): a frame is everything behind T
            if x.shape[2] != frames:
                raise ValueError("%s: x has %d frames, frames = %d" % (what, x.shape[2], frames))
            frame_elems = x[0, 0, 0].numel()
        elif x.dim() == 3:                                   # (B, C * T, hw)
            frame_elems = x.shape[2]
        else:
            raise ValueError("%s: x must be (B, C, T, ...) or (B, C * T, hw) for known frames" % what)
        if n % (frames * frame_elems) != 0:
            raise ValueError("%s: %d elements per sample are no multiple of %d frames x %d" % (what, n, frames, frame_elems))
        if tuple(frame_mask.shape) != (batch, frames):
            raise ValueError("%s: frame_mask must be (%d, %d), got %s" % (what, batch, frames, tuple(frame_mask.shape)))
        k.frame_mask, k.frames, k.frame_elems = _p(frame_mask), frames, frame_elems
    k.known, k.known_noise, k.level = _p(known), _p(known_noise), _p(level) if need_level else None
    return k


NOISE_STREAM_XT, NOISE_STREAM_KNOWN, NOISE_STREAM_STEP = 0, 1, 2       # counter word `stream` of the counter-based noise (csrc/lfdm_philox.h)


def check_seeds(seeds, batch, what="seeds"):
    """The list of `batch` Python ints in [0, 2^64) that `seeds` holds; ValueError otherwise (before anything is launched)."""
    try:
        seeds = list(seeds)
    except TypeError:
        raise ValueError("%s: a sequence of %d integers in [0, 2^64) is needed, got %r" % (what, batch, seeds))
    if len(seeds) != batch:
        raise ValueError("%s: %d seeds for %d videos (one per video)" % (what, len(seeds), batch))
    for v in seeds:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < (1 << 64):
            raise ValueError("%s: every seed must be an integer in [0, 2^64), got %r" % (what, v))
    return seeds


def seeds_tensor(seeds, device, out=None):
    """Unsigned 64-bit seeds as the int64 device tensor the kernels read (two's complement: the same 64 bits).  out: refilled in place."""
    t = torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in check_seeds(seeds, len(seeds))], dtype=torch.int64)
    if out is None:
        return t.to(device)
    return out.copy_(t)


def _seed_operand(what, lib, seeds, batch, device):
    if not torch.is_tensor(seeds):
        seeds = seeds_tensor(check_seeds(seeds, batch, what), device)
    if seeds.dtype != torch.int64 or tuple(seeds.shape) != (batch,) or not seeds.is_contiguous() or seeds.device != torch.device(device):
        raise ValueError("%s: seeds must be %d Python ints or a contiguous int64 tensor of %d words on the operands' device" % (what, batch, batch))
    if (lib.kind == "hip") != seeds.is_cuda:
        raise RuntimeError("%s: seeds on the wrong device for the %s library" % (what, lib.kind))
    return seeds


def _philox_fill(name, out, seeds, stream, step, window):
    lib = _lib()
    if out.dim() < 1 or out.numel() == 0:
        raise ValueError("%s: out must be (B, ...)" % name)
    batch = out.shape[0]
    n = out.numel() // batch
    item = out[0]
    if not item.is_contiguous() or (batch > 1 and out.stride(0) < n):
        raise ValueError("%s: every row of out must be dense and rows must not overlap, got strides %s" % (name, tuple(out.stride())))
    if (lib.kind == "hip") != out.is_cuda:
        raise RuntimeError("%s: out on the wrong device for the %s library (no CPU fallback exists)" % (name, lib.kind))
    if stream not in (NOISE_STREAM_XT, NOISE_STREAM_KNOWN, NOISE_STREAM_STEP):
        raise ValueError("%s: stream must be 0 (x_T), 1 (known-frame noise) or 2 (step noise), got %r" % (name, stream))
    if not (0 <= int(step) < 1 << 32 and 0 <= int(window) < 1 << 32):
        raise ValueError("%s: step and window are 32-bit counter words" % name)
    seeds = _seed_operand(name, lib, seeds, batch, out.device)
    fn = lib.lfdm_philox_normal_f32 if name == "philox_normal" else lib.lfdm_philox_bits_u32
    lib.check(fn(_p(out), _p(seeds), batch, n, out.stride(0) if batch > 1 else n, int(stream), int(step), int(window), _stream(lib)),
              "lfdm_" + name)
    return out


def philox_normal(out, seeds, *, stream, step=0, window=0):
    """lfdm_philox_normal_f32: fills the float32 tensor out (B, ...) - dense rows, any row stride - with the counter-based standard normals
    of the videos `seeds` (B Python ints in [0, 2^64), or an int64 device tensor of the same bits): row b is a function of
    (seeds[b], window, stream, step) alone."""
    if out.dtype != torch.float32:
        raise TypeError("philox_normal: out must be float32, got %s" % out.dtype)
    return _philox_fill("philox_normal", out, seeds, stream, step, window)


def philox_bits(out, seeds, *, stream, step=0, window=0):
    """lfdm_philox_bits_u32: the raw Philox4x32-10 words behind philox_normal, as the bits of the int32 tensor out (B, ...): element i of a row
    is output i & 3 of the counter (i >> 2, step, stream, window) under the key of the row's seed."""
    if out.dtype != torch.int32:
        raise TypeError("philox_bits: out must be int32 (the raw 32-bit words), got %s" % out.dtype)
    return _philox_fill("philox_bits", out, seeds, stream, step, window)


def _sampler_step(lib, x, eps, coef, step_dev, quantile, advance, x0_out, ws, known, **operands):
    """The one call behind sampler_step / sampler_step_ms (operands already checked): fills lfdm_sampler_step_params - `known` the checked
    KnownOperands, `operands` the fields that select the update (noise | hist, multistep | seeds, window)."""
    batch = x.shape[0]
    n = x.numel() // batch
    if ws is None:
        ws = sampler_ws(batch, n, x.device)
    p = _native.SamplerStepParams(x=_p(x), eps=_p(eps), x0_out=_p(x0_out), batch=batch, n=n, coef=_p(coef), step_dev=_p(step_dev),
                                  quantile=quantile, advance=int(advance), ws=_p(ws), ws_bytes=ws.numel() * 4, known=known, **operands)
    lib.check(lib.lfdm_sampler_step_f32(C.byref(p), _stream(lib)), "lfdm_sampler_step_f32")
    return x


def sampler_step(x, eps, noise, coef, step_dev, *, quantile=0.9, advance=True, x0_out=None, ws=None,
                 known=None, known_noise=None, frame_mask=None, level=None, frames=None, seeds=None, window=None, elem_mask=None):
    """lfdm_sampler_step_f32, the DDIM / DDPM update.  With the five known-frame keywords (all or none): frames whose frame_mask[b, t] is set
    are stored as level[step + 1] = (a, s) applied to (known, known_noise) instead of the update's result.
    seeds (int64 device tensor (B), ops.seeds_tensor) + window (int32 device tensor of one word), both or none, with noise=None: the step
    noise is computed inside the update kernel from (seeds[b], window, step) and is bit for bit what
    philox_normal(stream=2, step=the step counter's value, window=window) writes.
    elem_mask (bool / uint8 of x's shape) in place of frame_mask / frames: one mask byte per element; passing both forms is
    refused."""
    lib = _lib()
    _chk(lib, x, eps, noise, coef, step_dev, x0_out, ws)
    k = _known_operands("sampler_step", x, known, known_noise, frame_mask, level, frames, elem_mask)
    if (seeds is None) != (window is None):
        raise ValueError("sampler_step: seeds and window go together (both or none)")
    if seeds is not None and noise is not None:
        raise ValueError("sampler_step: seeds (noise computed in the kernel) and a noise tensor exclude each other")
    if seeds is not None:
        seeds = _seed_operand("sampler_step", lib, seeds, x.shape[0], x.device)
        if not torch.is_tensor(window) or window.dtype != torch.int32 or window.numel() != 1 or window.device != x.device:
            raise ValueError("sampler_step: window must be an int32 tensor of one word on x's device")
    return _sampler_step(lib, x, eps, coef, step_dev, quantile, advance, x0_out, ws, k, noise=_p(noise), seeds=_p(seeds), window=_p(window))


def sampler_step_ms(x, eps, hist, coef, step_dev, *, quantile=0.9, advance=True, x0_out=None, ws=None,
                    known=None, known_noise=None, frame_mask=None, level=None, frames=None, elem_mask=None):
    """lfdm_sampler_step_f32 with multistep set: x <- k_x*x + k_m*m + k_prev*hist, hist <- m (the thresholded data prediction of this step);
    coef rows {c_x, c_eps, k_x, k_m, k_prev, 0} (GaussianDiffusion._ms_step_tables).  Known-frame keywords as sampler_step."""
    lib = _lib()
    _chk(lib, x, eps, hist, coef, step_dev, x0_out, ws)
    k = _known_operands("sampler_step_ms", x, known, known_noise, frame_mask, level, frames, elem_mask)
    if hist.numel() != x.numel():
        raise ValueError("sampler_step_ms: hist must have x's %d elements, got %d" % (x.numel(), hist.numel()))
    return _sampler_step(lib, x, eps, coef, step_dev, quantile, advance, x0_out, ws, k, hist=_p(hist), multistep=1)


def _known_blend(what, x, a, s, known, known_noise, **mask):
    lib = _lib()
    _chk(lib, x, known, known_noise)
    if known is None or known_noise is None or any(v is None for v in mask.values()):
        raise ValueError("%s: known, known_noise and %s are required" % (what, " and ".join(mask)))
    k = _known_operands(what, x, known, known_noise, mask.get("frame_mask"), None, mask.get("frames"), mask.get("elem_mask"), need_level=False)
    batch = x.shape[0]
    lib.check(lib.lfdm_known_blend_f32(_p(x), C.byref(k), float(a), float(s), batch, x.numel() // batch, _stream(lib)), "lfdm_known_blend_f32")
    return x


def known_blend(x, known, known_noise, frame_mask, a, s, frames):
    """lfdm_known_blend_f32: x[b, :, t] <- a * known + s * known_noise where frame_mask[b, t] (the x_T blend of a conditioned video)."""
    return _known_blend("known_blend", x, a, s, known, known_noise, frame_mask=frame_mask, frames=frames)


def known_blend_elem(x, known, known_noise, elem_mask, a, s):
    """lfdm_known_blend_f32 with an element mask: x[e] <- a * known[e] + s * known_noise[e] where elem_mask[e] (bool / uint8 of x's shape): the
    x_T blend of an element-conditioned video and, with an all-True mask, the entry of a schedule on a given latent."""
    if any(t is not None and t.data_ptr() == x.data_ptr() for t in (known, known_noise)):
        raise ValueError("known_blend_elem: x must not alias known or known_noise")
    return _known_blend("known_blend_elem", x, a, s, known, known_noise, elem_mask=elem_mask)


# ---------------------------------------------------------------------------------------------
# DM training with known frames / elements held clean (csrc/train_diffusion.hip)
# ---------------------------------------------------------------------------------------------

LOSS_TYPES = {"l1": 0, "l2": 1}         # LFDM_LOSS_L1 / LFDM_LOSS_L2
OBJECTIVES = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}           # LFDM_OBJ_NOISE / _X0 / _V
_OBJECTIVE_NEEDS = {"pred_noise": ("noise",), "pred_x0": ("x_start",), "pred_v": ("x_start", "noise")}
_LOSS_TICKETS = {}                      # device -> the zeroed ticket word lfdm_objective_loss_fwd_f32 leaves zeroed


def _train_operands(what, lib, like, floats, t=None, tables=()):
    """The dense float32 (B, ...) operands of the three training entry points (all of `like`'s shape and device), the (B,) int64 device
    tensor t and the schedule tables; -> (batch, n)."""
    if like.dim() < 2 or like.numel() == 0:
        raise ValueError("%s: operands must be (B, ...) and not empty" % what)
    for name, v in floats.items():
        if not torch.is_tensor(v) or v.dtype != torch.float32 or tuple(v.shape) != tuple(like.shape) or v.device != like.device:
            raise ValueError("%s: %s must be a float32 tensor of shape %s on the operands' device" % (what, name, tuple(like.shape)))
    _chk(lib, *floats.values(), *tables)
    _dense(*floats.values(), *tables)
    batch = like.shape[0]
    if t is not None:
        if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (batch,) or not t.is_contiguous() or t.device != like.device:
            raise ValueError("%s: t must be a contiguous (%d,) int64 tensor on the operands' device (it is read there)" % (what, batch))
        if len({tuple(v.shape) for v in tables}) != 1 or tables[0].dim() != 1 or any(v.dtype != torch.float32 or v.device != like.device for v in tables):
            raise ValueError("%s: the schedule tables must be float32 vectors of one length on the operands' device" % what)
    return batch, like.numel() // batch


def _train_mask(what, x, frame_mask, elem_mask, frames):
    """lfdm_train_mask of the three mask forms: none | frame_mask (B, frames) | elem_mask of x's shape; bool or uint8, used as bytes.  A
    frame of a planar (B, C, T, ...) operand is everything behind T, of (B, C * T, hw) one row."""
    if frame_mask is None and elem_mask is None:
        if frames is not None:
            raise ValueError("%s: frames needs frame_mask" % what)
        return _native.TrainMask()
    if frame_mask is not None and elem_mask is not None:
        raise ValueError("%s: frame_mask and elem_mask exclude each other" % what)
    mask = frame_mask if elem_mask is None else elem_mask
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or not mask.is_contiguous() or mask.device != x.device:
        raise ValueError("%s: the mask must be a contiguous bool / uint8 tensor on the operands' device" % what)
    batch = x.shape[0]
    n = x.numel() // batch
    if elem_mask is not None:
        if frames is not None:
            raise ValueError("%s: elem_mask has no frame split" % what)
        if tuple(elem_mask.shape) != tuple(x.shape):
            raise ValueError("%s: elem_mask must have the operands' shape %s, got %s" % (what, tuple(x.shape), tuple(elem_mask.shape)))
        return _native.TrainMask(elem_mask=_p(elem_mask))
    if x.dim() >= 4:
        frames = x.shape[2] if frames is None else int(frames)
        if x.shape[2] != frames:
            raise ValueError("%s: the operands have %d frames, frames = %d" % (what, x.shape[2], frames))
        frame_elems = n // (x.shape[1] * frames)              # (everything behind T, without three views to count it)
    elif x.dim() == 3 and frames is not None:
        frames, frame_elems = int(frames), x.shape[2]
    else:
        raise ValueError("%s: operands must be (B, C, T, ...) or, with frames, (B, C * T, hw) for a frame mask" % what)
    if frames < 1 or n % (frames * frame_elems) != 0:
        raise ValueError("%s: %d elements per sample are no multiple of %d frames x %d" % (what, n, frames, frame_elems))
    if tuple(frame_mask.shape) != (batch, frames):
        raise ValueError("%s: frame_mask must be (%d, %d), got %s" % (what, batch, frames, tuple(frame_mask.shape)))
    return _native.TrainMask(_p(frame_mask), None, frames, frame_elems)


def _loss_code(what, loss_type):
    if loss_type not in LOSS_TYPES:
        raise ValueError("%s: loss_type must be 'l1' or 'l2', got %r" % (what, loss_type))
    return LOSS_TYPES[loss_type]


def _train_dest(what, t, shape, like):
    if t is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=like.device)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != like.device:
        raise ValueError("%s: a destination must be a contiguous float32 tensor of shape %s on the operands' device" % (what, tuple(shape)))
    return t


def train_qsample(x_start, noise, t, a_tab, s_tab, *, frame_mask=None, elem_mask=None, frames=None, out=None):
    """lfdm_train_qsample_f32: x_noisy = known ? x_start : a_tab[t_b] * x_start + s_tab[t_b] * noise - the bits of q_sample's expression on
    the unknown elements, the bits of x_start on the known ones.  t: (B,) int64 on the device (read there, clamped to the tables); a_tab /
    s_tab: sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod.  Mask: none, frame_mask (B, T) or elem_mask of x_start's shape."""
    lib = _lib()
    out = _train_dest("train_qsample", out, x_start.shape, x_start)
    batch, n = _train_operands("train_qsample", lib, x_start, dict(x_start=x_start, noise=noise, out=out), t, (a_tab, s_tab))
    mask = _train_mask("train_qsample", x_start, frame_mask, elem_mask, frames)
    lib.check(lib.lfdm_train_qsample_f32(_p(x_start), _p(noise), _p(t), _p(a_tab), _p(s_tab), a_tab.numel(), C.byref(mask), _p(out), batch, n,
                                         _stream(lib)), "lfdm_train_qsample_f32")
    return out


def _addr(t):
    return None if t is None else t.data_ptr()          # (a pointer field of a ctypes struct takes the integer)


def _loss_params(what, lib, objective, loss_type, x_start, noise, out, floats, t, a_tab, s_tab, r_tab, m_tab, w_tab):
    """What the two directions of the loss share -> lfdm_train_loss_params with the objective, the checked (B, ...) operands (`floats`: what
    the caller calls them -> tensor, `out` among them), t and the tables filled in.  x_start / noise may be None where the objective does not
    use them (they are never read); a table that is None stays null (w_tab None: weight 1; the masked backward reads none and has no t)."""
    code = _loss_code(what, loss_type)
    if objective not in OBJECTIVES:
        raise ValueError("%s: objective must be one of %s, got %r" % (what, tuple(OBJECTIVES), objective))
    floats.update({k: v for k, v in (("x_start", x_start), ("noise", noise)) if v is not None})
    missing = [k for k in _OBJECTIVE_NEEDS[objective] if k not in floats]
    if missing:
        raise ValueError("%s: objective %r needs %s (pred_noise: noise; pred_x0: x_start; pred_v: x_start and noise)"
                         % (what, objective, " and ".join(missing)))
    tables = tuple(v for v in (a_tab, s_tab, r_tab, m_tab, w_tab) if v is not None)
    batch, n = _train_operands(what, lib, out, floats, t, tables)
    return _native.TrainLossParams(objective=OBJECTIVES[objective], loss_type=code, x_start=_addr(x_start), noise=_addr(noise), out=_addr(out),
                                   t=_addr(t), a_tab=_addr(a_tab), s_tab=_addr(s_tab), r_tab=_addr(r_tab), m_tab=_addr(m_tab), w_tab=_addr(w_tab),
                                   t_len=tables[0].numel() if tables else 0, batch=batch, n=n)


def _loss_fwd(what, objective, x_start, noise, out, floats, x_noisy, t, a_tab, s_tab, r_tab, m_tab, w_tab, loss_type, frame_mask, elem_mask, frames,
              loss, inv_count, sample_loss, pred_x0, means=True):
    """The one forward behind masked_loss_fwd and objective_loss_fwd -> (loss, inv_count, sample_loss, pred_x0).  means=False: the per-sample
    means go to scratch behind the workspace (sample_loss is a required output of the kernel) and None comes back in their place."""
    lib = _lib()
    pred_x0 = _train_dest(what, pred_x0, out.shape, out)
    floats.update(x_noisy=x_noisy, pred_x0=pred_x0)
    p = _loss_params(what, lib, objective, loss_type, x_start, noise, out, floats, t, a_tab, s_tab, r_tab, m_tab, w_tab)
    batch = p.batch
    loss, inv_count = _train_dest(what, loss, (1,), out), _train_dest(what, inv_count, (batch,), out)
    if means:
        sample_loss = _train_dest(what, sample_loss, (batch,), out)
    p.mask = _train_mask(what, out, frame_mask, elem_mask, frames)
    nbytes = lib.lfdm_masked_loss_ws_bytes(batch, p.n)
    ws = torch.empty(nbytes // 8 + (0 if means else (batch + 1) // 2), dtype=torch.int64, device=out.device)
    ticket = _LOSS_TICKETS.get(out.device)
    if ticket is None:
        ticket = _LOSS_TICKETS[out.device] = torch.zeros(1, dtype=torch.int32, device=out.device)
    p.x_noisy, p.loss, p.inv_count, p.pred_x0 = x_noisy.data_ptr(), loss.data_ptr(), inv_count.data_ptr(), pred_x0.data_ptr()
    p.sample_loss = sample_loss.data_ptr() if means else ws.data_ptr() + nbytes
    p.ws, p.ws_bytes, p.ticket = ws.data_ptr(), nbytes, ticket.data_ptr()
    lib.check(lib.lfdm_objective_loss_fwd_f32(C.byref(p), _stream(lib)), "lfdm_objective_loss_fwd_f32")
    return loss, inv_count, sample_loss, pred_x0


def _loss_bwd(what, objective, x_start, noise, out, floats, t, a_tab, s_tab, w_tab, inv_count, gout, loss_type, frame_mask, elem_mask, frames,
              dout):
    """The one backward behind masked_loss_bwd and objective_loss_bwd -> d loss / d out."""
    lib = _lib()
    dout = _train_dest(what, dout, out.shape, out)
    floats.update(dout=dout)
    p = _loss_params(what, lib, objective, loss_type, x_start, noise, out, floats, t, a_tab, s_tab, None, None, w_tab)
    for name, v, count in (("inv_count", inv_count, p.batch), ("gout", gout, 1)):
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.numel() != count or not v.is_contiguous() or v.device != out.device:
            raise ValueError("%s: %s must be a contiguous float32 tensor of %d element(s) on the operands' device" % (what, name, count))
    p.mask = _train_mask(what, out, frame_mask, elem_mask, frames)
    p.inv_count, p.gout, p.dout = inv_count.data_ptr(), gout.data_ptr(), dout.data_ptr()
    lib.check(lib.lfdm_objective_loss_bwd_f32(C.byref(p), _stream(lib)), "lfdm_objective_loss_bwd_f32")
    return dout


def masked_loss_fwd(noise, pred, x_noisy, t, r_tab, m_tab, *, loss_type="l1", frame_mask=None, elem_mask=None, frames=None, loss=None,
                    inv_count=None, pred_x0=None):
    """The masked loss (lfdm_objective_loss_fwd_f32 with LFDM_OBJ_NOISE and no weights) -> (loss (1,), inv_count (B,), pred_x0): loss =
    (1 / B) sum_b S_b / max(N_b, 1) with S_b the sum of |noise - pred| ('l2': squared) over the UNKNOWN elements of sample b and N_b their
    number; inv_count[b] = 1 / max(N_b, 1) (the backward's operand); pred_x0 = r_tab[t_b] * x_noisy - m_tab[t_b] * pred, x_noisy where known
    (r_tab / m_tab: sqrt_recip_alphas_cumprod / sqrt_recipm1_alphas_cumprod).  Fixed summation order: the same bits on every run."""
    loss, inv_count, _, pred_x0 = _loss_fwd("masked_loss_fwd", "pred_noise", None, noise, pred, dict(pred=pred), x_noisy, t, None, None, r_tab, m_tab,
                                            None, loss_type, frame_mask, elem_mask, frames, loss, inv_count, None, pred_x0, means=False)
    return loss, inv_count, pred_x0


def masked_loss_bwd(noise, pred, inv_count, gout, *, loss_type="l1", frame_mask=None, elem_mask=None, frames=None, out=None):
    """The masked loss's backward (lfdm_objective_loss_bwd_f32 with LFDM_OBJ_NOISE and no weights): dpred = -sign(noise - pred) * gout *
    inv_count[b] / B ('l2': 2 (pred - noise) in place of the sign), exactly 0.0 at every known element.  gout: one float32 on the device
    (read there)."""
    return _loss_bwd("masked_loss_bwd", "pred_noise", None, noise, pred, dict(pred=pred), None, None, None, None, inv_count, gout, loss_type,
                     frame_mask, elem_mask, frames, out)


def objective_loss_fwd(objective, x_start, noise, out, x_noisy, t, a_tab, s_tab, r_tab, m_tab, w_tab=None, *, loss_type="l1", frame_mask=None,
                       elem_mask=None, frames=None, loss=None, inv_count=None, sample_loss=None, pred_x0=None):
    """lfdm_objective_loss_fwd_f32 -> (loss (1,), inv_count (B,), sample_loss (B,), pred_x0): masked_loss_fwd for a training objective
     - `out` is the denoiser's output, target = noise | x_start | a * noise - s * x_start for "pred_noise" | "pred_x0" |
    "pred_v", pred_x0 = r * x_noisy - m * out | out | a * x_noisy - s * out (x_noisy where known) - with the per-timestep weight w_tab[t_b]
    (None: 1) on each sample's mean: loss = (1 / B) sum_b w_b S_b / max(N_b, 1); sample_loss[b] = S_b / max(N_b, 1), unweighted.  x_start
    ("pred_noise") / noise ("pred_x0") may be None and are never read.  "pred_noise" without w_tab: the bits of masked_loss_fwd."""
    return _loss_fwd("objective_loss_fwd", objective, x_start, noise, out, dict(out=out), x_noisy, t, a_tab, s_tab, r_tab, m_tab, w_tab, loss_type,
                     frame_mask, elem_mask, frames, loss, inv_count, sample_loss, pred_x0)


def objective_loss_bwd(objective, x_start, noise, out, t, a_tab, s_tab, w_tab, inv_count, gout, *, loss_type="l1", frame_mask=None,
                       elem_mask=None, frames=None, dout=None):
    """lfdm_objective_loss_bwd_f32: d loss / d out = c_b * d |target - out| / d out with c_b = ((gout * inv_count[b]) * w_tab[t_b]) / B in
    fp32 (w_tab None: no product), the target recomputed from x_start / noise; exactly 0.0 at every known element.  "pred_noise" without
    w_tab: the bits of masked_loss_bwd."""
    return _loss_bwd("objective_loss_bwd", objective, x_start, noise, out, dict(out=out), t, a_tab, s_tab, w_tab, inv_count, gout, loss_type,
                     frame_mask, elem_mask, frames, dout)


# ---------------------------------------------------------------------------------------------
# progressive distillation: the teacher's step with a row per sample and the student's target (csrc/distill.hip)
# ---------------------------------------------------------------------------------------------

def _distill_table(what, name, tab, cols, row, batch, like):
    """A (rows, cols) float32 coefficient table and its (B,) int64 row index, both on the operands' device; -> rows."""
    if not torch.is_tensor(tab) or tab.dtype != torch.float32 or tab.dim() != 2 or tab.shape[1] != cols or tab.shape[0] < 1 \
            or not tab.is_contiguous() or tab.device != like.device:
        raise ValueError("%s: %s must be a contiguous (rows >= 1, %d) float32 table on the operands' device" % (what, name, cols))
    if not torch.is_tensor(row) or row.dtype != torch.int64 or tuple(row.shape) != (batch,) or not row.is_contiguous() or row.device != like.device:
        raise ValueError("%s: the row index of %s must be a contiguous (%d,) int64 tensor on the operands' device (it is read there)"
                         % (what, name, batch))
    return tab.shape[0]


def distill_x0(x, out, coef, row, x0=None):
    """lfdm_distill_x0_f32: x0[b] = c_x x[b] - c_eps out[b] with (c_x, c_eps) = coef[row[b]][0:2] - the eager fp32 expression's bits; a
    coefficient that is exactly 0 skips its operand, which may then hold NaN ("pred_x0" rows {0, -1}: the bits of out).  coef: a (rows, 6)
    step table; row: (B,) int64 on the device (read there, clamped to the table).  The operand of `abs_quantile` under dynamic thresholding."""
    lib = _lib()
    x0 = _train_dest("distill_x0", x0, x.shape, x)
    batch, n = _train_operands("distill_x0", lib, x, dict(x=x, out=out, x0=x0))
    _chk(lib, coef)
    rows = _distill_table("distill_x0", "coef", coef, 6, row, batch, x)
    lib.check(lib.lfdm_distill_x0_f32(_p(x), _p(out), _p(coef), _p(row), rows, _p(x0), batch, n, _stream(lib)), "lfdm_distill_x0_f32")
    return x0


def distill_step(x, out, coef, row, thr=None, x_next=None, *, x_ref=None, tcoef=None, trow=None, x_target=None, eps_target=None):
    """lfdm_distill_step_f32: one DDIM step (eta = 0) with a coefficient row per sample, {c_x, c_eps, k_x0, k_eps, k_x, -} = coef[row[b]]:
        x0 = c_x x - c_eps out;  s = 1 (thr None: the static clamp) or max(thr[b], 1);  m = clamp(x0, -s, s) / s
        v = k_x0 m [+ k_eps out] [+ k_x x]  -> x_next (made here when None; may be x itself)
    thr: (B,) float32, `abs_quantile` of `distill_x0`.  Target mode - x_ref, tcoef ((rows, 4) {q0, q1, q2, q3}), trow ((B,) int64) together,
    x_target / eps_target made here when None: xt = q0 v + q1 x_ref, et = q2 x_ref + q3 xt; x_next may then stay None and v is not stored.
    -> x_next, or (x_next | None, x_target, eps_target) in target mode."""
    lib = _lib()
    what = "distill_step"
    given = [v is not None for v in (x_ref, tcoef, trow)]
    if any(given) != all(given) or (not any(given) and (x_target is not None or eps_target is not None)):
        raise ValueError("%s: x_ref, tcoef and trow go together, and x_target / eps_target only with them" % what)
    target = all(given)
    floats = dict(x=x, out=out)
    if not target or x_next is not None:
        x_next = floats["x_next"] = _train_dest(what, x_next, x.shape, x)
    if target:
        x_target = _train_dest(what, x_target, x.shape, x)
        eps_target = _train_dest(what, eps_target, x.shape, x)
        floats.update(x_ref=x_ref, x_target=x_target, eps_target=eps_target)
    batch, n = _train_operands(what, lib, x, floats)
    _chk(lib, coef, tcoef, thr)
    rows = _distill_table(what, "coef", coef, 6, row, batch, x)
    trows = _distill_table(what, "tcoef", tcoef, 4, trow, batch, x) if target else 0
    if thr is not None and (not torch.is_tensor(thr) or thr.dtype != torch.float32 or tuple(thr.shape) != (batch,) or not thr.is_contiguous()
                            or thr.device != x.device):
        raise ValueError("%s: thr must be a contiguous (%d,) float32 tensor on the operands' device" % (what, batch))
    lib.check(lib.lfdm_distill_step_f32(_p(x), _p(out), _p(coef), _p(row), rows, _p(thr), _p(x_next), _p(x_ref), _p(tcoef), _p(trow), trows,
                                        _p(x_target), _p(eps_target), batch, n, _stream(lib)), "lfdm_distill_step_f32")
    return (x_next, x_target, eps_target) if target else x_next


def cfg_combine(cond_eps, null_eps, scale, out):
    lib = _lib()
    _chk(lib, cond_eps, null_eps, out)
    lib.check(lib.lfdm_cfg_combine_f32(_p(cond_eps), _p(null_eps), float(scale), _p(out), cond_eps.numel(),
                                       _stream(lib)), "lfdm_cfg_combine_f32")
    return out


def cfg_rescale_ws(batch, n, device):
    """Workspace of cfg_combine_rescale for (batch, n) operands: lfdm_cfg_rescale_ws_bytes, as doubles; no initialisation, no state."""
    nbytes = _lib().lfdm_cfg_rescale_ws_bytes(batch, n)
    if nbytes == 0:
        raise ValueError("cfg_rescale_ws: needs batch > 0 and n >= 2 elements per sample, got batch %r, n %r" % (batch, n))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def cfg_combine_rescale(cond, null, scale, phi, out, ws=None, factor_out=None):
    """lfdm_cfg_combine_rescale_f32: out = g * (phi * std(cond) / std(g) + 1 - phi) with g = null + (cond - null) * scale (cfg_combine's
    bits) and both standard deviations per sample - dim 0 - over all of its n elements, unbiased, in double (Lin et al. 2024, DESIGN.md
    4.15).  cond / null / out: dense float32 of one shape (batch, ...); out may be cond or null.  phi in [0, 1]; 0 gives cfg_combine's
    bits.  ws: cfg_rescale_ws(batch, n) (made here when None; any tensor of enough bytes).  factor_out: None or (batch,) float32, the
    factor each sample was multiplied by.  Two launches, no atomics: the same bits on every run, whatever the batch around a sample."""
    lib = _lib()
    _chk(lib, cond, null, out, factor_out)
    for name, t in (("cond", cond), ("null", null), ("out", out)):
        if t.dtype != torch.float32 or t.dim() < 1 or tuple(t.shape) != tuple(cond.shape) or not t.is_contiguous():
            raise ValueError("cfg_combine_rescale: %s must be a dense float32 tensor of cond's shape %s" % (name, tuple(cond.shape)))
    batch = cond.shape[0]
    n = cond.numel() // batch if batch else 0
    if factor_out is not None and (factor_out.dtype != torch.float32 or factor_out.numel() != batch or not factor_out.is_contiguous()):
        raise ValueError("cfg_combine_rescale: factor_out must be a dense float32 tensor of %d element(s)" % batch)
    if ws is None:
        ws = cfg_rescale_ws(batch, n, cond.device)
    elif ws.device != cond.device or not ws.is_contiguous():
        raise ValueError("cfg_combine_rescale: ws must be a dense tensor on the operands' device")
    lib.check(lib.lfdm_cfg_combine_rescale_f32(_p(cond), _p(null), float(scale), float(phi), _p(out), _p(factor_out), batch, n, _p(ws),
                                               ws.numel() * ws.element_size(), _stream(lib)), "lfdm_cfg_combine_rescale_f32")
    return out


def abs_quantile(x, quantile=0.9, ws=None):
    lib = _lib()
    batch = x.shape[0]
    n = x.numel() // batch
    _chk(lib, x, ws)
    if ws is None:
        ws = sampler_ws(batch, n, x.device)
    out = torch.empty(batch, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_abs_quantile_f32(_p(x), batch, n, quantile, _p(out), _p(ws), ws.numel() * 4,
                                        _stream(lib)), "lfdm_abs_quantile_f32")
    return out


def _warp_params(src, out, batch, frames, h, w, c, flow_x, flow_y, occ, fh, fw, fsb, fst, prev,
                 occ_scale, occ_bias, ld_src, ld_prev, ld_out, prev_is_cl):
    p = WarpParams()
    p.src, p.prev, p.out = _p(src), _p(prev), _p(out)
    p.batch, p.frames, p.h, p.w, p.c = batch, frames, h, w, c
    p.ld_src, p.ld_prev, p.ld_out = ld_src, ld_prev, ld_out
    p.flow_x, p.flow_y, p.occ = _p(flow_x), _p(flow_y), _p(occ)
    p.fh, p.fw, p.fsb, p.fst = fh, fw, fsb, fst
    p.occ_scale, p.occ_bias, p.prev_is_cl = occ_scale, occ_bias, int(prev_is_cl)
    return p


def warp_cl(src, batch, frames, h, w, flow_x, flow_y, occ, fh, fw, fsb, fst, *, prev=None,
            occ_scale=1.0, occ_bias=0.0, out=None):
    """src: CL (batch*h*w, C); out/prev: CL (batch*frames*h*w, C). flow_x/flow_y/occ: tensors whose
    data_ptr is the map base (element (b,t,y,x) at b*fsb + t*fst + y*fw + x)."""
    lib = _lib()
    _chk(lib, src, flow_x, flow_y, occ, prev, out)
    c = src.shape[1]
    if out is None:
        out = torch.empty(batch * frames * h * w, c, dtype=torch.float32, device=src.device)
    p = _warp_params(src, out, batch, frames, h, w, c, flow_x, flow_y, occ, fh, fw, fsb, fst, prev,
                     occ_scale, occ_bias, _ld(src), _ld(prev) if prev is not None else 0,
                     _ld(out), True)
    lib.check(lib.lfdm_warp_cl_f32(C.byref(p), _stream(lib)), "lfdm_warp_cl_f32")
    return out


def warp_planar(src, frames, flow_x, flow_y, occ, fh, fw, fsb, fst, *, prev=None, prev_is_cl=False,
                occ_scale=1.0, occ_bias=0.0, out=None):
    """src: planar (B, C, H, W); out: planar (B, C, frames, H, W)."""
    lib = _lib()
    _chk(lib, src, flow_x, flow_y, occ, prev, out)
    b, c, h, w = src.shape
    assert src.is_contiguous()
    if out is None:
        out = torch.empty(b, c, frames, h, w, dtype=torch.float32, device=src.device)
    ld_prev = _ld(prev) if (prev is not None and prev_is_cl) else 0
    p = _warp_params(src, out, b, frames, h, w, c, flow_x, flow_y, occ, fh, fw, fsb, fst, prev,
                     occ_scale, occ_bias, 0, ld_prev, 0, prev_is_cl)
    lib.check(lib.lfdm_warp_planar_f32(C.byref(p), _stream(lib)), "lfdm_warp_planar_f32")
    return out


def affine_act_cl(x, a, b, act=ACT_RELU, out=None):
    lib = _lib()
    _chk(lib, x, a, b, out)
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_affine_act_cl_f32(_p(x), _p(out), x.shape[0], x.shape[1], _ld(x),
                                         _ld(out), _p(a), _p(b), act, _stream(lib)), "lfdm_affine_act_cl_f32")
    return out


def avgpool2_cl(x, n_img, h, w, out=None):
    lib = _lib()
    _chk(lib, x, out)
    assert x.is_contiguous()
    c = x.shape[1]
    if out is None:
        out = torch.empty(n_img * (h // 2) * (w // 2), c, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_avgpool2_cl_f32(_p(x), _p(out), n_img, h, w, c, _stream(lib)), "lfdm_avgpool2_cl_f32")
    return out


def planar_to_cl(x, n_img, channels, hw, out=None):
    lib = _lib()
    _chk(lib, x, out)
    if out is None:
        out = torch.empty(n_img * hw, channels, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_planar_to_cl_f32(_p(x), _p(out), n_img, channels, hw, _ld(out), _stream(lib)),
              "lfdm_planar_to_cl_f32")
    return out


def cl_to_planar(x, n_img, channels, hw, out=None):
    lib = _lib()
    _chk(lib, x, out)
    if out is None:
        out = torch.empty(n_img, channels, hw, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_cl_to_planar_f32(_p(x), _p(out), n_img, channels, hw, _ld(x), _stream(lib)),
              "lfdm_cl_to_planar_f32")
    return out


def depthwise_down_planar(x, weight, stride, pad_lo, pad_hi):
    """AntiAliasInterpolation2d core: x (N,C,H,W) planar, weight (C,1,k,k) -> (N,C,Ho,Wo)."""
    lib = _lib()
    x = x.contiguous()
    wt = weight.reshape(weight.shape[0], weight.shape[-2], weight.shape[-1]).contiguous()
    _chk(lib, x, wt)
    n, c, h, w = x.shape
    k = wt.shape[-1]
    ho = (h + pad_lo + pad_hi - k + 1 + stride - 1) // stride
    wo = (w + pad_lo + pad_hi - k + 1 + stride - 1) // stride
    out = torch.empty(n, c, ho, wo, dtype=torch.float32, device=x.device)
    lib.check(lib.lfdm_depthwise_down_planar_f32(_p(x), _p(wt), _p(out), n, c, h, w, k, pad_lo, pad_hi, stride, _stream(lib)),
              "lfdm_depthwise_down_planar_f32")
    return out


# ---------------------------------------------------------------------------------------------
# uint8 preview strips of a sampled video (csrc/render.hip)
# ---------------------------------------------------------------------------------------------
PANELS = ("source", "out", "warped", "flow", "conf")          # LFDM_PANEL_* = the position in this tuple
_ident_cache = {}


def _chk_dev(lib, *tensors):
    """_chk's device rule for operands that are not all fp32 / int32."""
    for t in tensors:
        if t is None:
            continue
        if lib.kind == "hip" and not t.is_cuda:
            raise RuntimeError("lfdm ops need tensors on the GPU (no CPU fallback exists)")
        if lib.kind == "emu" and t.is_cuda:
            raise RuntimeError("emulation library needs CPU tensors")


def _identity_table(s, device):
    """torch.linspace(-1, 1, s), the call io_compat.get_grid makes, on `device` (made on the host, kept per size and device)."""
    key = (int(s), str(device))
    if key not in _ident_cache:
        _ident_cache[key] = torch.linspace(-1.0, 1.0, int(s)).to(device)
    return _ident_cache[key]


def flow_to_color_u8(grid, out=None):
    """lfdm_flow_color_u8: grid (B, 2, T, s, s) fp32 sampling grid (x, y) -> (B * T, s, s, 3) uint8, io_compat.flow_to_color(grid -
    identity) of every frame (what misc.flow2fig colours), the identity from torch.linspace(-1, 1, s).  grid may be the first two
    channels of a (B, 3, T, s, s) latent: only the batch stride may differ from a contiguous tensor's."""
    lib = _lib()
    _chk_dev(lib, grid, out)
    if grid.dtype != torch.float32 or grid.dim() != 5 or grid.shape[1] != 2 or grid.shape[3] != grid.shape[4]:
        raise ValueError("flow_to_color_u8: grid must be a float32 (B, 2, T, s, s) tensor, got %s %s" % (grid.dtype, tuple(grid.shape)))
    b, _, t, s, _ = grid.shape
    if s % 4 != 0:
        raise ValueError("flow_to_color_u8: s = %d is not a multiple of 4" % s)
    if tuple(grid.stride()[1:]) != (t * s * s, s * s, s, 1) or (b > 1 and grid.stride(0) < 2 * t * s * s):
        grid = grid.contiguous()
    stride = grid.stride(0) if b > 1 else 2 * t * s * s
    if out is None:
        out = torch.empty(b * t, s, s, 3, dtype=torch.uint8, device=grid.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (b * t, s, s, 3) or not out.is_contiguous() or out.device != grid.device:
        raise ValueError("flow_to_color_u8: out must be a contiguous uint8 (%d, %d, %d, 3) tensor on grid's device" % (b * t, s, s))
    lib.check(lib.lfdm_flow_color_u8(_p(grid), stride, _p(_identity_table(s, grid.device)), _p(out), b, t, s, _stream(lib)),
              "lfdm_flow_color_u8")
    return out


def render_strip(*, source=None, out_vid=None, warped_vid=None, flow_color=None, conf=None, mean=(0.0, 0.0, 0.0),
                 panels=PANELS, indexed=False, out=None):
    """lfdm_render_strip_u8: the per-frame panel strip of the demo scripts, (B, T, S, P * S, 3) uint8 RGB - or (B, T, S, P * S) uint8
    indices into io_compat.STRIP_PALETTE when indexed - for the ordered panel names in `panels` (from ops.PANELS).  Operands (only those
    of the listed panels are needed): source (B, 3, S, S), out_vid / warped_vid (B, 3, T, S, S), conf (B, 1, T, s, s) fp32,
    flow_color (B * T, s, s, 3) uint8 from flow_to_color_u8; S = 4 s.  Image panels are io_compat.sample_img with `mean`, conf is
    io_compat.conf2fig, flow is the colour image resized like io_compat.flow2fig does - to the byte."""
    lib = _lib()
    panels = tuple(panels)
    for p in panels:
        if p not in PANELS:
            raise ValueError("render_strip: unknown panel %r (one of %s)" % (p, ", ".join(PANELS)))
    if not 1 <= len(panels) <= 8:
        raise ValueError("render_strip: 1 to 8 panels, got %d" % len(panels))
    ops_by_name = dict(source=source, out=out_vid, warped=warped_vid, flow=flow_color, conf=conf)
    used = {p: ops_by_name[p] for p in panels}
    for p, t in used.items():
        if t is None:
            raise ValueError("render_strip: panel %r needs its operand" % p)
    _chk_dev(lib, out, *used.values())
    # batch, frame count and size: from a video operand, else conf, else flow_color + source (given ones count, listed or not)
    vid = out_vid if out_vid is not None else warped_vid
    if vid is not None and vid.dim() == 5:
        b, frames, size = vid.shape[0], vid.shape[2], vid.shape[-1]
    elif conf is not None and conf.dim() == 5:
        b, frames, size = conf.shape[0], conf.shape[2], 4 * conf.shape[-1]
    elif flow_color is not None and source is not None and flow_color.dim() == 4 and source.dim() == 4:
        b, size = source.shape[0], 4 * flow_color.shape[1]
        frames = flow_color.shape[0] // b
    else:
        raise ValueError("render_strip: the frame count needs out_vid, warped_vid or conf (or flow_color together with source)")
    s = size // 4
    want = dict(source=(b, 3, size, size), out=(b, 3, frames, size, size), warped=(b, 3, frames, size, size),
                flow=(b * frames, s, s, 3), conf=(b, 1, frames, s, s))
    for p, t in used.items():
        dt = torch.uint8 if p == "flow" else torch.float32
        if t.dtype != dt or tuple(t.shape) != want[p] or not t.is_contiguous():
            raise ValueError("render_strip: %s must be a contiguous %s tensor of shape %s, got %s %s"
                             % (p, dt, want[p], t.dtype, tuple(t.shape)))
    if size != 4 * s or s % 4 != 0:
        raise ValueError("render_strip: frame size %d must be 4 x a latent size that is a multiple of 4" % size)
    mean = [float(m) for m in mean]
    if len(mean) != 3:
        raise ValueError("render_strip: mean has three channels")
    dev = next(iter(used.values())).device
    shape = (b, frames, size, len(panels) * size) + (() if indexed else (3,))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError("render_strip: out must be a contiguous uint8 %s tensor on the operands' device" % (shape,))
    import numpy as np
    add = (C.c_double * 3)(*(np.array(mean) / 255.0).tolist())          # io_compat.sample_img's `np.array(mean) / 255.0`
    codes = (C.c_int * len(panels))(*[PANELS.index(p) for p in panels])
    lib.check(lib.lfdm_render_strip_u8(_p(used.get("source")), _p(used.get("out")), _p(used.get("warped")), _p(used.get("flow")),
                                       _p(used.get("conf")), add, codes, len(panels), int(bool(indexed)), _p(out), b, frames, size, s,
                                       _stream(lib)), "lfdm_render_strip_u8")
    return out


# ---------------------------------------------------------------------------------------------
# paired video metrics
# ---------------------------------------------------------------------------------------------

METRIC_DOMAINS = ("raw", "unit", "uint8")          # LFDM_METRIC_* = the position in this tuple
SSIM_WINDOW = 11


def _metric_table(what, out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != device:
        raise ValueError("%s: out must be a contiguous float64 %s tensor on the operands' device" % (what, shape))
    return out


def video_metrics(a, b, *, mean=(0, 0, 0), domain="unit", out=None):
    """lfdm_video_metrics: a, b (B, C, T, H, W) fp32 videos -> (B, T, 3) float64, [l1, mse, ssim] of every frame averaged over its
    channels (1 <= C <= 4; H, W >= 11, any value).  domain: "raw" the values as they are; "unit" io_compat.sample_img before its
    scaling, clamp(float32(x + mean / 255), 0, 1); "uint8" the bytes the demo writes, over 255.  SSIM is Wang et al.'s (11-tap Gaussian,
    sigma 1.5, valid interior only) with data range 1 in every domain, "raw" included.  All arithmetic is fp64 in a fixed order: a
    frame's numbers are bit-identical from run to run and whatever the batch around it."""
    lib = _lib()
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("video_metrics: %s must be a float32 tensor, got %s" % (name, getattr(t, "dtype", type(t))))
    if domain not in METRIC_DOMAINS:
        raise ValueError("video_metrics: unknown domain %r (one of %s)" % (domain, ", ".join(METRIC_DOMAINS)))
    if a.dim() != 5 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("video_metrics: a and b must be (B, C, T, H, W) tensors of one shape, got %s and %s"
                         % (tuple(a.shape), tuple(b.shape)))
    bsz, ch, frames, h, w = a.shape
    if bsz < 1 or frames < 1 or not 1 <= ch <= 4:
        raise ValueError("video_metrics: needs B, T >= 1 and 1 <= C <= 4, got %s" % (tuple(a.shape),))
    if h < SSIM_WINDOW or w < SSIM_WINDOW:
        raise ValueError("video_metrics: H, W must be at least %d (the SSIM window), got %s" % (SSIM_WINDOW, tuple(a.shape)))
    mean = [float(m) for m in mean]
    if len(mean) != ch:
        raise ValueError("video_metrics: mean has %d values for %d channels (shape %s)" % (len(mean), ch, tuple(a.shape)))
    if a.device != b.device:
        raise ValueError("video_metrics: a is on %s, b on %s" % (a.device, b.device))
    _chk_dev(lib, a, b, out)
    out = _metric_table("video_metrics", out, (bsz, frames, 3), a.device)
    a = a if a.is_contiguous() else a.contiguous()
    b = b if b.is_contiguous() else b.contiguous()
    ws_bytes = lib.lfdm_video_metrics_ws_bytes(bsz, ch, frames, h, w)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=a.device)
    import numpy as np
    add = (C.c_double * ch)(*(np.array(mean) / 255.0).tolist())          # io_compat.sample_img's `np.array(mean) / 255.0`
    lib.check(lib.lfdm_video_metrics(_p(a), _p(b), add, METRIC_DOMAINS.index(domain), _p(out), bsz, ch, frames, h, w, _p(ws), ws_bytes,
                                     _stream(lib)), "lfdm_video_metrics")
    return out


def _flow_grid(g):
    """(tensor, batch stride) of a (B, 2, T, s, s) grid: copied only when more than its batch stride differs from a contiguous one's."""
    b, _, t, s, _ = g.shape
    if tuple(g.stride()[1:]) != (t * s * s, s * s, s, 1) or (b > 1 and g.stride(0) < 2 * t * s * s):
        g = g.contiguous()
    return g, (g.stride(0) if b > 1 else 2 * t * s * s)


def flow_metrics(grid_a, grid_b, conf_a=None, conf_b=None, out=None):
    """lfdm_flow_metrics: two sampling grids (B, 2, T, s, s) fp32 (x, y) and optionally their confidences (B, 1, T, s, s) ->
    (B, T, 2) float64: [mean end-point error sqrt(dx^2 + dy^2) in the grids' normalised units, mean |conf_a - conf_b| (0 without
    confidences)] per frame.  A grid may be the first two channels of a (B, 3, T, s, s) latent: only the batch stride may differ
    from a contiguous tensor's.  fp64 in a fixed order, like video_metrics."""
    lib = _lib()
    if (conf_a is None) != (conf_b is None):
        raise ValueError("flow_metrics: give both confidences or neither")
    for name, t in (("grid_a", grid_a), ("grid_b", grid_b), ("conf_a", conf_a), ("conf_b", conf_b)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise TypeError("flow_metrics: %s must be a float32 tensor, got %s" % (name, getattr(t, "dtype", type(t))))
    if grid_a.dim() != 5 or grid_a.shape[1] != 2 or grid_a.shape[3] != grid_a.shape[4] or tuple(grid_a.shape) != tuple(grid_b.shape):
        raise ValueError("flow_metrics: grids must be (B, 2, T, s, s) tensors of one shape, got %s and %s"
                         % (tuple(grid_a.shape), tuple(grid_b.shape)))
    b, _, t, s, _ = grid_a.shape
    if b < 1 or t < 1 or not 1 <= s <= 4096:
        raise ValueError("flow_metrics: needs B, T >= 1 and 1 <= s <= 4096, got %s" % (tuple(grid_a.shape),))
    for name, c in (("conf_a", conf_a), ("conf_b", conf_b)):
        if c is not None and tuple(c.shape) != (b, 1, t, s, s):
            raise ValueError("flow_metrics: %s must be %s, got %s" % (name, (b, 1, t, s, s), tuple(c.shape)))
    for x in (grid_b, conf_a, conf_b):
        if x is not None and x.device != grid_a.device:
            raise ValueError("flow_metrics: operands on %s and %s" % (grid_a.device, x.device))
    _chk_dev(lib, grid_a, grid_b, conf_a, conf_b, out)
    out = _metric_table("flow_metrics", out, (b, t, 2), grid_a.device)
    grid_a, stride_a = _flow_grid(grid_a)
    grid_b, stride_b = _flow_grid(grid_b)
    if conf_a is not None:
        conf_a = conf_a if conf_a.is_contiguous() else conf_a.contiguous()
        conf_b = conf_b if conf_b.is_contiguous() else conf_b.contiguous()
    lib.check(lib.lfdm_flow_metrics(_p(grid_a), stride_a, _p(grid_b), stride_b, _p(conf_a), _p(conf_b), _p(out), b, t, s, _stream(lib)),
              "lfdm_flow_metrics")
    return out


def psnr(mse_table, out=None):
    """lfdm_psnr_f64: 10 log10(1 / mse) elementwise over a float64 table (data range 1), inf where mse == 0."""
    lib = _lib()
    if not isinstance(mse_table, torch.Tensor) or mse_table.dtype != torch.float64:
        raise TypeError("psnr: the table must be a float64 tensor, got %s" % getattr(mse_table, "dtype", type(mse_table)))
    _chk_dev(lib, mse_table, out)
    src = mse_table if mse_table.is_contiguous() else mse_table.contiguous()
    out = _metric_table("psnr", out, tuple(src.shape), src.device)
    if src.numel():
        lib.check(lib.lfdm_psnr_f64(_p(src), _p(out), src.numel(), _stream(lib)), "lfdm_psnr_f64")
    return out


# ---------------------------------------------------------------------------------------------
# training batches from a packed uint8 frame store (csrc/video_prep.hip)
# ---------------------------------------------------------------------------------------------
PREP_RATIOS = (1, 2, 4)
PREP_STATS, PREP_MAIN = 1, 2          # LFDM_PREP_*


def _prep_operands(what, rows_name, store_u8, rows, params, hue_shift, valid, image_size, jitter, outs, frames=None):
    """The operand checks video_prep and frame_pairs_prep share: the store, the (B, T) table of store rows (T == frames when given), every
    row range-checked on the host, and with jitter the factor tables and the valid rectangles.  Uploads the small tables and allocates
    the stats workspace.  -> (lib, N, S, H, B, T, device, rows, params, hue_shift, valid, ws, ws_bytes)."""
    lib = _lib()
    if not isinstance(store_u8, torch.Tensor) or store_u8.dtype != torch.uint8 or store_u8.dim() != 4 or store_u8.shape[3] != 3 \
            or store_u8.shape[1] != store_u8.shape[2] or not store_u8.is_contiguous():
        raise ValueError("%s: store_u8 must be a contiguous uint8 (N, S, S, 3) tensor, got %s %s"
                         % (what, getattr(store_u8, "dtype", type(store_u8)), tuple(getattr(store_u8, "shape", ()))))
    _chk_dev(lib, store_u8, *[o for o in outs if isinstance(o, torch.Tensor)])
    n, s = int(store_u8.shape[0]), int(store_u8.shape[1])
    h = int(image_size)
    if s % 4 != 0 or h % 4 != 0 or h < 4:
        raise ValueError("%s: store_size %d and image_size %d must be multiples of 4" % (what, s, h))
    if h * (s // h) != s or s // h not in PREP_RATIOS:
        raise ValueError("%s: store_size / image_size must be 1, 2 or 4, got %d / %d" % (what, s, h))
    if n < 1:
        raise ValueError("%s: the store is empty" % what)
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.numel() == 0 \
            or (frames is not None and rows.shape[1] != frames):
        raise ValueError("%s: %s must be a non-empty int32 (B, %s) tensor, got %s %s"
                         % (what, rows_name, "T" if frames is None else frames, getattr(rows, "dtype", type(rows)),
                            tuple(getattr(rows, "shape", ()))))
    b, t = int(rows.shape[0]), int(rows.shape[1])
    lo, hi = int(rows.min()), int(rows.max())
    if lo < 0 or hi >= n:
        raise IndexError("%s: %s holds %d .. %d, the store has rows 0 .. %d" % (what, rows_name, lo, hi, n - 1))
    dev = store_u8.device

    def table(name, x):          # the small per-batch tables may come from the host: checked there, then uploaded
        if x is None or x.device == dev:
            return x if x is None else x.contiguous()
        if x.is_cuda:
            raise ValueError("%s: %s is on %s, the store on %s" % (what, name, x.device, dev))
        return x.contiguous().to(dev, non_blocking=True)

    rows = table(rows_name, rows)
    ws, ws_bytes = None, 0
    if jitter:
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or tuple(params.shape) != (b, 3):
            raise ValueError("%s: params must be a float32 (%d, 3) tensor" % (what, b))
        if not bool(torch.isfinite(params).all()):          # a NaN or inf factor would reach the kernel's float -> int conversion
            raise ValueError("%s: params holds a NaN or an infinity" % what)
        if not isinstance(hue_shift, torch.Tensor) or hue_shift.dtype != torch.int32 or tuple(hue_shift.shape) != (b,):
            raise ValueError("%s: hue_shift must be an int32 (%d,) tensor" % (what, b))
        if valid is not None:
            if not isinstance(valid, torch.Tensor) or valid.dtype != torch.int32 or tuple(valid.shape) != (b, 4):
                raise ValueError("%s: valid must be an int32 (%d, 4) tensor of (y0, x0, h, w)" % (what, b))
            vv = valid.cpu()
            if bool((vv < 0).any()) or bool((vv[:, 2:] < 1).any()) or bool(((vv[:, :2] + vv[:, 2:]) > s).any()):
                raise ValueError("%s: a valid rectangle is empty or leaves the %d x %d stored frame" % (what, s, s))
        params, hue_shift, valid = table("params", params), table("hue_shift", hue_shift), table("valid", valid)
        ws_bytes = lib.lfdm_video_prep_ws_bytes(b, t)
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    else:
        params = hue_shift = valid = None
    return lib, n, s, h, b, t, dev, rows, params, hue_shift, valid, ws, ws_bytes


def video_prep(store_u8, frame_index, params, hue_shift, mean, image_size, jitter, out=None, *, valid=None,
               launches=PREP_STATS | PREP_MAIN):
    """lfdm_video_prep_u8: gathers frames from store_u8 (N, S, S, 3) uint8 by frame_index (B, T) int32 and returns the training batch
    (B, 3, T, H, H) float32, H = image_size, S / H in {1, 2, 4}: bit for bit what data.FrameFolderVideos makes of the same pixels -
    data.color_jitter with the factors params (B, 3) float32 = (brightness, contrast, saturation) and hue_shift (B,) int32 = int(hf * 255)
    when `jitter`, the area shrink, - mean (3 floats, host), / 255.  jitter=False carries no jitter arithmetic at all (params and hue_shift
    may be None).  valid (B, 4) int32 = (y0, x0, h, w): the picture inside a zero-padded stored frame (non-square videos); jitter and the
    contrast mean see only it.  frame_index may have repeats and any order; every entry is range-checked here, on the host.  The four
    small tables (frame_index, params, hue_shift, valid) may be host tensors - they are checked there and uploaded - which avoids the
    read-back that checking a device tensor costs.  launches: measurement only (tools/bench_video_prep.py)."""
    lib, n, s, h, b, t, dev, frame_index, params, hue_shift, valid, ws, ws_bytes = _prep_operands(
        "video_prep", "frame_index", store_u8, frame_index, params, hue_shift, valid, image_size, jitter, (out,))
    mean = [float(m) for m in mean]
    if len(mean) != 3:
        raise ValueError("video_prep: mean has three channels")
    shape = (b, 3, t, h, h)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError("video_prep: out must be a contiguous float32 %s tensor on the store's device" % (shape,))
    lib.check(lib.lfdm_video_prep_u8(_p(store_u8), n, _p(frame_index), _p(params), _p(hue_shift), _p(valid), (C.c_float * 3)(*mean),
                                     _p(out), b, t, s, h, int(bool(jitter)), int(launches), _p(ws), ws_bytes, _stream(lib)),
              "lfdm_video_prep_u8")
    return out


def frame_pairs_prep(store_u8, pair_index, params, hue_shift, flip, image_size, jitter, out=None, *, valid=None):
    """lfdm_frame_pairs_prep_u8: LFAE stage-1 training pairs from store_u8 (N, S, S, 3) uint8 - returns (source, driving), each
    (B, 3, H, H) float32, bit for bit what lfae_train.FramePairs makes of the same pixels.  pair_index (B, 2) int32: the store rows of
    (source, driving), equal rows and any order allowed.  params, hue_shift, valid and jitter as in video_prep: one jitter per pair.
    flip (B,) int32 of 0 / 1: mirror both frames of the item left to right after shrink and padding (valid stays in unflipped
    coordinates).  No mean: / 255 only.  out: a pair of contiguous (B, 3, H, H) float32 tensors to write into.  The checks, and the
    small tables that may be host tensors, are video_prep's."""
    outs = (None, None) if out is None else tuple(out)
    if len(outs) != 2:
        raise ValueError("frame_pairs_prep: out is a (source, driving) pair of tensors")
    lib, n, s, h, b, _, dev, pair_index, params, hue_shift, valid, ws, ws_bytes = _prep_operands(
        "frame_pairs_prep", "pair_index", store_u8, pair_index, params, hue_shift, valid, image_size, jitter, outs, frames=2)
    if not isinstance(flip, torch.Tensor) or flip.dtype != torch.int32 or tuple(flip.shape) != (b,):
        raise ValueError("frame_pairs_prep: flip must be an int32 (%d,) tensor of 0 / 1" % b)
    if bool(((flip != 0) & (flip != 1)).any()):
        raise ValueError("frame_pairs_prep: flip holds a value other than 0 and 1")
    if flip.device != dev:
        if flip.is_cuda:
            raise ValueError("frame_pairs_prep: flip is on %s, the store on %s" % (flip.device, dev))
        flip = flip.to(dev, non_blocking=True)
    flip = flip.contiguous()
    shape = (b, 3, h, h)
    res = []
    for name, o in zip(("source", "driving"), outs):
        if o is None:
            o = torch.empty(shape, dtype=torch.float32, device=dev)
        elif not isinstance(o, torch.Tensor) or o.dtype != torch.float32 or tuple(o.shape) != shape or not o.is_contiguous() \
                or o.device != dev or o.data_ptr() % 16 != 0:
            raise ValueError("frame_pairs_prep: out (%s) must be a contiguous, 16-byte aligned float32 %s tensor on the store's device"
                             % (name, shape))
        res.append(o)
    lib.check(lib.lfdm_frame_pairs_prep_u8(_p(store_u8), n, _p(pair_index), _p(params), _p(hue_shift), _p(valid), _p(flip), _p(res[0]),
                                           _p(res[1]), b, s, h, int(bool(jitter)), _p(ws), ws_bytes, _stream(lib)),
              "lfdm_frame_pairs_prep_u8")
    return res[0], res[1]


# ---------------------------------------------------------------------------------------------
# temporal resampling of a sampled latent (csrc/latent_resample.hip)
# ---------------------------------------------------------------------------------------------
RESAMPLE_MODES = ("linear", "cubic")          # LFDM_RESAMPLE_* = the position in this tuple


def resample_tables(times, frames):
    """The host side of lfdm_latent_resample_f32's time tables: times (a sequence or host tensor of floats in [0, frames - 1], any order,
    repeats allowed, at least one) -> (idx int32 array, frac float32 array), time = idx + frac with frac in [0, 1).  i = floor(t) and
    a = t - i are taken in float64, a is rounded to fp32, and an a that rounds to 1.0f becomes (i + 1, 0): the kernel converts no time."""
    import numpy as np
    if isinstance(times, torch.Tensor):
        if times.is_cuda:
            raise ValueError("latent_resample: times is a host sequence or host tensor (it is checked on the host), got a tensor on %s"
                             % times.device)
        times = times.detach().reshape(-1).to(torch.float64).numpy()
    try:
        t = np.asarray(list(times) if not isinstance(times, np.ndarray) else times, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("latent_resample: times must be a sequence of numbers")
    if t.size == 0:
        raise ValueError("latent_resample: times is empty (at least one output frame)")
    if not np.isfinite(t).all():
        raise ValueError("latent_resample: times holds a NaN or an infinity")
    if t.min() < 0.0 or t.max() > frames - 1:
        raise IndexError("latent_resample: times span %g .. %g, the latent has frames 0 .. %d (no extrapolation)"
                         % (t.min(), t.max(), frames - 1))
    i = np.floor(t)
    a = (t - i).astype(np.float32)
    up = a >= np.float32(1.0)
    i = i.astype(np.int64) + up
    a[up] = 0.0
    assert i.min() >= 0 and i.max() <= frames - 1 and not (a[i == frames - 1] != 0).any()
    return i.astype(np.int32), a


def _resample_call(what, latent, times, mode, clamp_from, maps, residual, out, conf):
    lib = _lib()
    if not isinstance(latent, torch.Tensor) or latent.dtype != torch.float32 or latent.dim() != 5:
        raise ValueError("%s: latent must be a float32 (B, C, T, H, W) tensor, got %s %s"
                         % (what, getattr(latent, "dtype", type(latent)), tuple(getattr(latent, "shape", ()))))
    _chk_dev(lib, latent, out, conf)
    b, c, t, h, w = (int(v) for v in latent.shape)
    if min(b, c, t, h, w) < 1:
        raise ValueError("%s: the latent is empty, shape %s" % (what, tuple(latent.shape)))
    if not latent.is_contiguous():
        raise ValueError("%s: the latent must be contiguous, got strides %s" % (what, tuple(latent.stride())))
    if (h * w) % 4 != 0:
        raise ValueError("%s: H * W = %d is not a multiple of 4" % (what, h * w))
    if mode not in RESAMPLE_MODES:
        raise ValueError("%s: unknown mode %r (one of %s)" % (what, mode, ", ".join(RESAMPLE_MODES)))
    if maps and c != 3:
        raise ValueError("%s: the maps form needs a latent of C == 3 channels (x, y, occlusion), got %d" % (what, c))
    clamp_from = c if clamp_from is None else int(clamp_from)
    if clamp_from < 0:
        raise ValueError("%s: clamp_from must be a channel index >= 0 (None: no clamp), got %d" % (what, clamp_from))
    idx, frac = resample_tables(times, t)
    n = int(idx.shape[0])
    if n > 65535 or b > 65535:
        raise ValueError("%s: at most 65535 output frames and batch elements per call, got %d and %d" % (what, n, b))
    dev = latent.device

    def result(name, x, shape):
        if x is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != shape or not x.is_contiguous() or x.device != dev:
            raise ValueError("%s: %s must be a contiguous float32 %s tensor on the latent's device" % (what, name, shape))
        return x

    out = result("out", out, (b, c, n, h, w))
    conf = result("conf", conf, (b, 1, n, h, w)) if maps else None
    for name, x in (("latent", latent), ("out", out), ("conf", conf)):
        if x is not None and x.data_ptr() % 16 != 0:
            raise ValueError("%s: %s is not 16-byte aligned" % (what, name))
    ident_x = _identity_table(w, dev) if maps and residual else None
    ident_y = _identity_table(h, dev) if maps and residual else None
    idx_d = torch.from_numpy(idx).to(dev, non_blocking=True)
    frac_d = torch.from_numpy(frac).to(dev, non_blocking=True)
    lib.check(lib.lfdm_latent_resample_f32(_p(latent), _p(idx_d), _p(frac_d), _p(ident_x), _p(ident_y), _p(out), _p(conf), b, c, t, n, h, w,
                                           RESAMPLE_MODES.index(mode), clamp_from, _stream(lib)), "lfdm_latent_resample_f32")
    return out, conf


def latent_resample(latent, times, mode="linear", clamp_from=None, out=None):
    """lfdm_latent_resample_f32: latent (B, C, T, H, W) fp32, contiguous -> (B, C, T', H, W), frame j taken at times[j] (resample_tables:
    floats in [0, T - 1], any order, repeats allowed).  mode "linear": x[i] + a (x[i+1] - x[i]); "cubic": Catmull-Rom with the end frames
    duplicated.  An integer time gives that frame bit for bit in both modes (selected: no other frame is read).  clamp_from: interpolated
    values of channels >= clamp_from are clamped to [-1, 1] (None: no clamp).  H * W % 4 == 0.  Everything is checked before the launch."""
    return _resample_call("latent_resample", latent, times, mode, clamp_from, False, False, out, None)[0]


def latent_resample_maps(latent, times, mode="linear", residual=False, clamp_from=None, out=None, conf=None):
    """latent_resample of a (B, 3, T, H, W) latent and FlowDiffusion._maps of the result in one launch -> (maps (B, 3, T', H, W), conf
    (B, 1, T', H, W)): maps = the resampled latent, with torch.linspace(-1, 1, .) added to channels 0 (x) and 1 (y) when `residual`
    (use_residual_flow); conf = (ch2 + 1) * 0.5.  At an integer time both are _maps(latent[:, :, i]) bit for bit."""
    return _resample_call("latent_resample_maps", latent, times, mode, clamp_from, True, bool(residual), out, conf)


# ---------------------------------------------------------------------------------------------
# joint sampling of a long video through overlapping windows (csrc/window_fold.hip)
# ---------------------------------------------------------------------------------------------
WINDOW_BLENDS = ("ramp", "uniform")
FOLD_MAX_CONTRIB = 8            # LFDM_FOLD_MAX_CONTRIB
JOINT_ELEMS_LIMIT = 1 << 24     # lfdm_sampler_step_f32's bound on the elements of one sample


def joint_windows(total_frames, frames, overlap, blend="ramp", *, channels=3, size=None):
    """The host tables of a joint long video: `total_frames` global frames covered by windows of `frames` frames.  -> (starts, table):
    starts (W,) int32 - 0, s, 2s, ... with s = frames - overlap while start + frames < total_frames, then one last window at
    total_frames - frames (total_frames <= frames: the single window [0] on a global latent of `frames` frames); table: dict of count (F,)
    int32, win / loc (F, 8) int32 and wgt (F, 8) float32 over the F = max(total_frames, frames) global frames - frame f's contributors in
    ascending window order, window number and frame inside it, and the weight p / sum p of the window profile p(t): "ramp"
    min(t + 1, frames - t), "uniform" 1 - formed in float64 and rounded once to fp32 (one contributor: exactly 1.0f).  Unused slots are
    zero.  Plain integers in, numpy arrays out; no device is needed.  size (keyword; the latent's S, with channels): also refuse a global
    latent the sampler update does not take."""
    import numpy as np
    for name, v in (("total_frames", total_frames), ("frames", frames), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("joint_windows: %s must be an integer, got %r" % (name, v))
    if blend not in WINDOW_BLENDS:
        raise ValueError("joint_windows: blend must be one of %s, got %r" % (WINDOW_BLENDS, blend))
    if total_frames < 1 or frames < 1:
        raise ValueError("joint_windows: total_frames and frames must be at least 1, got %d and %d" % (total_frames, frames))
    if not 1 <= overlap <= frames - 1:
        raise ValueError("joint_windows: overlap must lie in [1, frames - 1 = %d], got %d" % (frames - 1, overlap))
    total = max(total_frames, frames)
    if size is not None and channels * size * size * total >= JOINT_ELEMS_LIMIT:
        raise ValueError("joint_windows: %d frames of %d x %d x %d are %d elements per video, the sampler step takes fewer than 2^24 = %d"
                         % (total, channels, size, size, channels * size * size * total, JOINT_ELEMS_LIMIT))
    stride, starts = frames - overlap, [0]
    while starts[-1] + frames < total:
        nxt = starts[-1] + stride
        starts.append(nxt if nxt + frames < total else total - frames)
    return np.asarray(starts, dtype=np.int32), fold_table(total, frames, starts, blend)


def fold_table(total_frames, frames, starts, blend="ramp"):
    """The contributor table of `joint_windows` for given window starts (ascending, every frame of 0 .. total_frames - 1 covered)."""
    import numpy as np
    if blend not in WINDOW_BLENDS:
        raise ValueError("joint_windows: blend must be one of %s, got %r" % (WINDOW_BLENDS, blend))
    total, starts = int(total_frames), [int(s) for s in starts]
    if any(not 0 <= s <= total - frames for s in starts) or any(a >= b for a, b in zip(starts, starts[1:])):
        raise ValueError("joint_windows: starts must ascend inside [0, %d], got %s" % (total - frames, starts))
    t = np.arange(frames, dtype=np.float64)
    profile = np.minimum(t + 1.0, frames - t) if blend == "ramp" else np.ones(frames, dtype=np.float64)
    count = np.zeros(total, dtype=np.int32)
    win = np.zeros((total, FOLD_MAX_CONTRIB), dtype=np.int32)
    loc = np.zeros((total, FOLD_MAX_CONTRIB), dtype=np.int32)
    wgt = np.zeros((total, FOLD_MAX_CONTRIB), dtype=np.float32)
    for f in range(total):
        who = [(w, f - s) for w, s in enumerate(starts) if s <= f < s + frames]
        if len(who) > FOLD_MAX_CONTRIB:
            raise ValueError("joint_windows: frame %d lies in %d windows, the fold takes at most %d contributors per frame (a smaller "
                             "overlap)" % (f, len(who), FOLD_MAX_CONTRIB))
        p = np.array([profile[tt] for _, tt in who], dtype=np.float64)
        count[f] = len(who)
        win[f, :len(who)] = [w for w, _ in who]
        loc[f, :len(who)] = [tt for _, tt in who]
        if not who:
            raise ValueError("joint_windows: frame %d lies in no window of starts %s" % (f, starts))
        wgt[f, :len(who)] = (p / p.sum()).astype(np.float32)
    return {"count": count, "win": win, "loc": loc, "wgt": wgt}


class WindowStarts:
    """The window starts of window_gather on a device, with the host copy the entry point checks.  A plan keeps one: a captured graph binds
    the device table's address, `fill` rewrites both in place."""

    def __init__(self, starts, device):
        self.host = _host_i32("window_gather: starts", starts, 1)
        self.dev = torch.from_numpy(self.host).to(device)

    def fill(self, starts):
        host = _host_i32("window_gather: starts", starts, 1)
        if host.shape != self.host.shape:
            raise ValueError("window_gather: %d starts into a table of %d" % (host.shape[0], self.host.shape[0]))
        self.host[...] = host
        self.dev.copy_(torch.from_numpy(self.host))
        return self


class WindowTable:
    """The contributor table of window_fold on a device (count, win, loc, wgt of `joint_windows`), with the host copy of count the entry
    point checks and host copies of win / loc for the checks made here.  `fill` rewrites all in place (same frame count)."""
    KEYS = ("count", "win", "loc", "wgt")

    def __init__(self, table, device):
        self.host = self._check(table)
        self.dev = {k: torch.from_numpy(v).to(device) for k, v in self.host.items()}

    @staticmethod
    def _check(table):
        import numpy as np
        count = _host_i32("window_fold: table count", table["count"], 1)
        shape = (count.shape[0], FOLD_MAX_CONTRIB)
        win, loc = (_host_i32("window_fold: table " + k, table[k], 2) for k in ("win", "loc"))
        wgt = np.ascontiguousarray(np.asarray(table["wgt"], dtype=np.float32))
        if win.shape != shape or loc.shape != shape or wgt.shape != shape:
            raise ValueError("window_fold: win, loc and wgt must be (%d, %d) tables" % shape)
        return {"count": count.copy(), "win": win.copy(), "loc": loc.copy(), "wgt": wgt.copy()}

    def fill(self, table):
        host = self._check(table)
        if host["count"].shape != self.host["count"].shape:
            raise ValueError("window_fold: a table of %d frames into one of %d" % (host["count"].shape[0], self.host["count"].shape[0]))
        for k in self.KEYS:
            self.host[k][...] = host[k]
            self.dev[k].copy_(torch.from_numpy(self.host[k]))
        return self


def _host_i32(what, values, dim):
    import numpy as np
    if isinstance(values, torch.Tensor):
        if values.is_cuda:
            raise ValueError("%s is a host sequence or array (it is checked on the host), got a tensor on %s" % (what, values.device))
        values = values.detach().numpy()
    try:
        arr = np.asarray(values)
        if arr.dtype.kind not in "iu" or arr.ndim != dim or arr.size == 0:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("%s must be a non-empty %d-D sequence of integers" % (what, dim))
    return np.ascontiguousarray(arr.astype(np.int32))


def _window_operand(what, name, t, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 5 or not t.is_contiguous() or \
            (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s: %s must be a contiguous float32 5-D tensor%s, got %s %s"
                         % (what, name, "" if shape is None else " of shape %s" % (tuple(shape),), getattr(t, "dtype", type(t)),
                            tuple(getattr(t, "shape", ()))))
    if min(t.shape) < 1:
        raise ValueError("%s: %s is empty, shape %s" % (what, name, tuple(t.shape)))


def window_gather(x, starts, frames, out=None):
    """lfdm_window_gather_f32: x (B, C, F, S, S') fp32, contiguous -> out (B * W, C, frames, S, S') with out[b * W + w, :, t] =
    x[b, :, starts[w] + t]: the windows of a joint long video, rows in b * W + w order.  starts: W integers in [0, F - frames] - a host
    sequence (uploaded by this call) or a `WindowStarts` (a plan's table: nothing is uploaded).  A pure copy; everything is checked
    before the launch."""
    lib = _lib()
    what = "window_gather"
    _window_operand(what, "x", x)
    if not isinstance(starts, WindowStarts):
        starts = WindowStarts(starts, x.device)
    b, c, total, h, w = (int(v) for v in x.shape)
    frames, nwin = int(frames), int(starts.host.shape[0])
    if not 1 <= frames <= total:
        raise ValueError("%s: windows of %d frames do not fit a latent of %d" % (what, frames, total))
    if int(starts.host.min()) < 0 or int(starts.host.max()) > total - frames:
        raise ValueError("%s: starts span %d .. %d, windows of %d frames start in [0, %d]"
                         % (what, int(starts.host.min()), int(starts.host.max()), frames, total - frames))
    shape = (b * nwin, c, frames, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _window_operand(what, "out", out, shape)
    _chk_dev(lib, x, out, starts.dev)
    if out.device != x.device or starts.dev.device != x.device:
        raise ValueError("%s: x, out and the starts table must share a device" % what)
    lib.check(lib.lfdm_window_gather_f32(_p(x), _p(starts.dev), C.c_void_p(starts.host.ctypes.data), _p(out), b, nwin, c, total, frames,
                                         h * w, _stream(lib)), "lfdm_window_gather_f32")
    return out


def window_fold(ew, table, out):
    """lfdm_window_fold_f32: ew (B * W, C, T, S, S') fp32 window outputs -> out (B, C, F, S, S'), out[b, :, f] = sum_j wgt[f, j] *
    ew[b * W + win[f, j], :, loc[f, j]] over the frame's count[f] contributors in ascending j, one product and one addition each (no
    fma); a frame with one contributor of weight 1.0f is the window's value bit for bit.  table: the dict `joint_windows` returns (uploaded
    by this call) or a `WindowTable` (a plan's).  W is taken from the shapes; every count, window number and frame is checked here."""
    lib = _lib()
    what = "window_fold"
    _window_operand(what, "ew", ew)
    _window_operand(what, "out", out)
    if not isinstance(table, WindowTable):
        table = WindowTable(table, ew.device)
    bw, c, frames, h, w = (int(v) for v in ew.shape)
    b, total = int(out.shape[0]), int(out.shape[2])
    host = table.host
    if tuple(out.shape) != (b, c, total, h, w) or bw % b != 0 or frames > total:
        raise ValueError("%s: out %s does not go with window outputs %s" % (what, tuple(out.shape), tuple(ew.shape)))
    nwin = bw // b
    if host["count"].shape[0] != total:
        raise ValueError("%s: a table of %d frames for an output of %d" % (what, host["count"].shape[0], total))
    if int(host["count"].min()) < 1 or int(host["count"].max()) > FOLD_MAX_CONTRIB:
        raise ValueError("%s: every frame needs 1 .. %d contributors, the table's counts span %d .. %d"
                         % (what, FOLD_MAX_CONTRIB, int(host["count"].min()), int(host["count"].max())))
    import numpy as np
    used = np.arange(FOLD_MAX_CONTRIB)[None, :] < host["count"][:, None]
    if (used & ((host["win"] < 0) | (host["win"] >= nwin) | (host["loc"] < 0) | (host["loc"] >= frames))).any():
        raise ValueError("%s: the table names a window outside 0 .. %d or a frame outside 0 .. %d" % (what, nwin - 1, frames - 1))
    _chk_dev(lib, ew, out, *table.dev.values())
    if out.device != ew.device or any(t.device != ew.device for t in table.dev.values()):
        raise ValueError("%s: ew, out and the table must share a device" % what)
    dev = table.dev
    lib.check(lib.lfdm_window_fold_f32(_p(ew), _p(dev["count"]), _p(dev["win"]), _p(dev["loc"]), _p(dev["wgt"]),
                                       C.c_void_p(host["count"].ctypes.data), _p(out), b, nwin, c, total, frames, h * w, _stream(lib)),
              "lfdm_window_fold_f32")
    return out


# ---------------------------------------------------------------------------------------------
# training latents gathered from a flow-latent store (csrc/latent_gather.hip)
# ---------------------------------------------------------------------------------------------
LATENT_DTYPES = (torch.float32, torch.float16)          # LFDM_LATENT_* = the position in this tuple


def latent_gather(store, rows, residual, out=None):
    """lfdm_latent_gather_f32: store (N, 3, h, w) float32 or float16, contiguous - the frozen LFAE's raw outputs per frame (grid x, grid y,
    occlusion map) - gathered by rows (B, T) int32 into the latent (B, 3, T, h, w) float32 the diffusion denoises: bit for bit
    FlowDiffusion._latent_of of the gathered rows (an fp16 store as store.float()) - channels 0 / 1 minus torch.linspace(-1, 1, .) when
    `residual` (use_residual_flow), a copy otherwise; channel 2 = occ * 2 - 1.  rows may have repeats and any order and may be a host
    tensor (checked there, then uploaded: no read-back); every entry is range-checked here, on the host, before anything is launched
    (ValueError).  h * w % 4 == 0."""
    lib = _lib()
    if not isinstance(store, torch.Tensor) or store.dtype not in LATENT_DTYPES or store.dim() != 4 or store.shape[1] != 3 \
            or not store.is_contiguous():
        raise ValueError("latent_gather: store must be a contiguous float32 or float16 (N, 3, h, w) tensor, got %s %s"
                         % (getattr(store, "dtype", type(store)), tuple(getattr(store, "shape", ()))))
    _chk_dev(lib, store, out)
    n, _, h, w = (int(v) for v in store.shape)
    if n < 1 or h < 1 or w < 1:
        raise ValueError("latent_gather: the store is empty, shape %s" % (tuple(store.shape),))
    if (h * w) % 4 != 0:
        raise ValueError("latent_gather: h * w = %d is not a multiple of 4" % (h * w))
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.numel() == 0:
        raise ValueError("latent_gather: rows must be a non-empty int32 (B, T) tensor, got %s %s"
                         % (getattr(rows, "dtype", type(rows)), tuple(getattr(rows, "shape", ()))))
    b, t = int(rows.shape[0]), int(rows.shape[1])
    if b > 65535 or t > 65535:
        raise ValueError("latent_gather: at most 65535 batch elements and frames per call, got %d and %d" % (b, t))
    lo, hi = int(rows.min()), int(rows.max())
    if lo < 0 or hi >= n:
        raise ValueError("latent_gather: rows holds %d .. %d, the store has rows 0 .. %d" % (lo, hi, n - 1))
    dev = store.device
    if rows.device != dev:
        if rows.is_cuda:
            raise ValueError("latent_gather: rows is on %s, the store on %s" % (rows.device, dev))
        rows = rows.contiguous().to(dev, non_blocking=True)
    rows = rows.contiguous()
    shape = (b, 3, t, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() \
            or out.device != dev:
        raise ValueError("latent_gather: out must be a contiguous float32 %s tensor on the store's device" % (shape,))
    for name, x in (("store", store), ("out", out)):
        if x.data_ptr() % 16 != 0:
            raise ValueError("latent_gather: %s is not 16-byte aligned" % name)
    ident_x = _identity_table(w, dev) if residual else None
    ident_y = _identity_table(h, dev) if residual else None
    lib.check(lib.lfdm_latent_gather_f32(_p(store), LATENT_DTYPES.index(store.dtype), n, _p(rows), _p(ident_x), _p(ident_y), _p(out), b, t,
                                         h, w, _stream(lib)), "lfdm_latent_gather_f32")
    return out
