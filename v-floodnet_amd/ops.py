"""Thin host wrappers: torch tensors in, one C-ABI kernel launch each.

Used by the engine (``engine.py``), the feature bank and the parity tests.  Every
function enqueues on the current HIP stream and returns without synchronising.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import ptr, stream, check, ConvDesc


_cfg_tiles = None


def conv_cfg_tiles():
    """(BM, BN) of every tile configuration of the library (a constant of the build: asked once)."""
    global _cfg_tiles
    if _cfg_tiles is None:
        L = _lib.lib()
        out = []
        for c in range(L.vfn_conv_cfg_count()):
            bm, bn = C.c_int(), C.c_int()
            L.vfn_conv_cfg_tile(c, C.byref(bm), C.byref(bn))
            out.append((bm.value, bn.value))
        _cfg_tiles = tuple(out)
    return _cfg_tiles


def conv_cfg_wk(cfg):
    """K groups per workgroup of a tile configuration (vfn_conv_cfg_wk): > 1 = split-K inside the workgroup."""
    return _lib.lib().vfn_conv_cfg_wk(int(cfg))


def conv_cfg_tpb(cfg):
    """K tiles per workgroup barrier of a tile configuration (vfn_conv_cfg_tpb)."""
    return _lib.lib().vfn_conv_cfg_tpb(int(cfg))


def conv_cfgs(mode, _cache={}):
    """Ids of the tile configurations that arithmetic mode ``mode`` (0 f32, 1 bf16, 2 bf16x3) accepts (vfn_conv_cfg_modes)."""
    mode = int(mode)
    if mode not in _cache:
        L = _lib.lib()
        _cache[mode] = tuple(c for c in range(L.vfn_conv_cfg_count()) if L.vfn_conv_cfg_modes(c) >> mode & 1)
    return _cache[mode]


def __getattr__(name):
    """``ops.BF16_CFGS``, the name the ids of the reduced-precision modes had as a literal: asked of the library on first use."""
    if name == 'BF16_CFGS':
        return conv_cfgs(1)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def conv_cfg_kind(cfg):
    """0 = LDS-tiled, 1 = wave-autonomous (conv_direct_kernel), 2 = stream-K (conv_streamk_kernel) -- vfn_conv_cfg_kind."""
    return _lib.lib().vfn_conv_cfg_kind(int(cfg))


SK_WS_FLOATS, SK_MAX_TILES = _lib.DEFINES['VFN_CONV_SK_WS_FLOATS'], _lib.DEFINES['VFN_CONV_SK_MAX_TILES']
_sk_scratch = {}


def streamk_scratch(device):
    """(workspace, counters) for stream-K launches made through the convenience wrappers (one pair per device; launches on
    one stream run one after the other, so they may share it)."""
    key = str(device)
    if key not in _sk_scratch:
        _sk_scratch[key] = (torch.empty(SK_WS_FLOATS, dtype=torch.float32, device=device),
                            torch.zeros(SK_MAX_TILES, dtype=torch.int32, device=device))
    return _sk_scratch[key]


def set_streamk(desc, workspace, counters):
    """A stream-K configuration (conv_cfg_kind == 2) needs its partial-tile workspace and zeroed tile counters."""
    assert workspace.numel() >= SK_WS_FLOATS and counters.numel() >= SK_MAX_TILES
    desc.ksplit, desc.split_from = 1, 0
    desc.partial, desc.tile_counters = ptr(workspace), ptr(counters)
    return desc


def conv_cfg_names(mode=0):
    """Kernel instantiation behind every tile configuration, as rocprofv3 prints it."""
    L = _lib.lib()
    out = []
    for c in range(L.vfn_conv_cfg_count()):
        v = [C.c_int() for _ in range(5)]
        L.vfn_conv_cfg_info(c, *[C.byref(x) for x in v])
        bm, bn, wm, wn, dma = [x.value for x in v]
        wk, tpb = L.vfn_conv_cfg_wk(c), L.vfn_conv_cfg_tpb(c)
        if L.vfn_conv_cfg_kind(c) > 0:
            buf = C.create_string_buffer(96)
            L.vfn_conv_cfg_name(c, buf, 96)
            out.append(buf.value.decode())
            continue
        out.append(f'conv_igemm_dma_kernel<{bm}, {bn}, {wm}, {wn}, {dma}>' if dma else
                   f'conv_igemm_wk_kernel<{bm}, {bn}, {wm}, {wn}, {wk}, {4 if tpb > 1 else 3}, {tpb}, {int(mode)}>' if (wk > 1 or tpb > 1) else
                   f'conv_igemm_kernel<{bm}, {bn}, {wm}, {wn}, {int(mode)}>')
    return out


def pad_rows(wp, mult=256):
    """Pad packed weights [Cout,K] with zero rows to a multiple of ``mult`` filters."""
    cout = wp.shape[0]
    cp = (cout + mult - 1) // mult * mult
    if cp == cout:
        return wp.contiguous()
    out = torch.zeros(cp, wp.shape[1], dtype=wp.dtype, device=wp.device)
    out[:cout] = wp
    return out


def pack_weights_lp(wp, mode):
    """f32 packed filters [cout_pad, K] -> the operand image the bf16 / bf16x3 conv kernels stage without conversion
    (vfn_conv_desc.w_packed = 1): mode 1: bf16 [cout_pad, K]; mode 2: per 32-channel K tile 32 hi then 32 lo bf16,
    x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (round to nearest even, as the kernels' own conversion)."""
    if mode == 1:
        return wp.to(torch.bfloat16).contiguous()
    assert mode == 2 and wp.shape[1] % 32 == 0
    hi = wp.to(torch.bfloat16)
    lo = (wp - hi.float()).to(torch.bfloat16)
    cp, K = wp.shape
    return torch.cat([hi.view(cp, K // 32, 32), lo.view(cp, K // 32, 32)], dim=2).contiguous()


def make_conv_desc(x, wp, cout, kh, kw, stride, pad, out, scale=None, shift=None, res=None,
                   relu_in=False, relu_out=False, cin=None, in_ld=None, out_ld=None, res_ld=None,
                   N=None, H=None, W=None):
    """x: NHWC [N,H,W,in_ld]; wp: [cout_pad, kh*kw*cin]; out: [N,Ho,Wo,out_ld] (or 2-D [M,out_ld])."""
    if N is None:
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
    in_ld = in_ld if in_ld is not None else x.shape[-1]
    cin = cin if cin is not None else in_ld
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    out_ld = out_ld if out_ld is not None else out.shape[-1]       # (out may be None with an image-only producer: pass out_ld)
    d = ConvDesc()
    d.inp, d.w, d.scale, d.shift, d.res, d.out = ptr(x), ptr(wp), ptr(scale), ptr(shift), ptr(res), ptr(out)
    d.N, d.H, d.W, d.Cin, d.in_ld = N, H, W, cin, in_ld
    d.Ho, d.Wo, d.Cout, d.cout_pad = Ho, Wo, cout, wp.shape[0]
    d.out_ld = out_ld
    d.res_ld = res_ld if res_ld is not None else (res.shape[-1] if res is not None else 0)
    d.KH, d.KW, d.stride, d.pad = kh, kw, stride, pad
    d.relu_in, d.relu_out = int(relu_in), int(relu_out)
    d.M = N * Ho * Wo
    d.ksplit, d.split_from, d.partial = 1, 0, None
    d.tile_counters = None
    d.res_mod = 0
    d.w_packed = 0
    d.in_lp, d.out_lp_relu, d.out_lp = 0, 0, None
    d.mask, d.mask_ld, d.mask_after = None, 0, 0
    d.w_batch_rows = 0
    assert wp.shape[1] == kh * kw * cin
    return d


def use_packed_weights(desc, w_lp):
    """Point the descriptor at filters from ``pack_weights_lp`` (keep ``w_lp`` alive: raw pointer)."""
    desc.w = ptr(w_lp)
    desc.w_packed = 1
    return desc


def set_splitk(desc, ksplit, workspace, split_from=0, rows=None, counters=None):
    """Cut the tiles from index ``split_from`` on along K into ``ksplit`` slices.  ``rows`` = output rows
    those tiles cover (default: all M); ``workspace``: float32 tensor with >= ksplit*rows*Cout elements;
    ``counters``: zeroed int32 tensor (one per split tile) -> the tile is reduced inside the same launch."""
    if ksplit > 1:
        rows = desc.M if rows is None else rows
        assert workspace is not None and workspace.numel() >= ksplit * rows * desc.Cout
        desc.ksplit, desc.split_from, desc.partial = int(ksplit), int(split_from), ptr(workspace)
        desc.tile_counters = ptr(counters) if counters is not None else None
    else:
        desc.ksplit, desc.split_from, desc.partial = 1, 0, None
        desc.tile_counters = None
    return desc


def tail_split_options(desc, bm, bn, max_split=8, mode=0):
    """(split_from, ksplit, rows) candidates that cut only the last partial round of tiles."""
    m_tiles = (desc.M + bm - 1) // bm
    n_tiles = (desc.Cout + bn - 1) // bn
    tiles = m_tiles * n_tiles
    out = []
    for unit in (256, 512):
        full = (tiles // unit) * unit
        full -= full % n_tiles
        if full <= 0 or full >= tiles:
            continue
        rows = desc.M - (full // n_tiles) * bm
        for ks in valid_splits(desc, max_split, mode)[1:]:
            out.append((full, ks, rows))
    return out


def valid_splits(desc, max_split=16, mode=0):
    """Split factors for which every K slice is non-empty and the epilogue can run vectorised."""
    nk = desc.KH * desc.KW * (desc.Cin // (64 if mode == 1 else 32))
    out = [1]
    if desc.Cout % 4 or desc.out_ld % 4 or (desc.res and desc.res_ld % 4):
        return out
    for s_ in range(2, max_split + 1):
        per = (nk + s_ - 1) // s_
        if per * (s_ - 1) < nk and per >= 4:
            out.append(s_)
    return out


# arithmetic of the matrix kernels: 0 exact f32, 1 bf16 operands, 2 bf16x3 (hi/lo split operands, 3 MFMAs per product)
MODES = {'fp32': 0, 'bf16': 1, 'bf16x3': 2}
_CONV_FN = ('vfn_conv2d_nhwc_f32', 'vfn_conv2d_nhwc_bf16', 'vfn_conv2d_nhwc_bf16x3')


# Configuration ids from WINO_GEMM_CFG0 on: a Winograd-domain GEMM descriptor (make_winograd_gemm_desc) launched as the PERSISTENT
# kernel (vfn_winograd_gemm_f32) instead of one workgroup per output tile: id = WINO_GEMM_CFG0 + tile cfg (0..7) + 8 * (workgroups / 128)
WINO_GEMM_CFG0 = 1000
WINO_GEMM_TILES = ((128, 128, 4, 2), (64, 128, 2, 4), (128, 64, 4, 2), (64, 64, 2, 2))


def wino_gemm_cfg(tile_cfg, wgs=512):
    return WINO_GEMM_CFG0 + int(tile_cfg) + 8 * (int(wgs) // 128)


# 32-row tiles of the f32 transform-domain GEMM (vfn_winograd_gemm_f32 configurations 8 + tile cfg): ids of their own range, same
# encoding: id = WINO_GEMM32_CFG0 + tile cfg (& 3: index into WINO_GEMM_TILES32, bit 2: request depth) + 8 * (workgroups / 128)
WINO_GEMM32_CFG0 = 1500
WINO_GEMM_TILES32 = ((32, 128, 1, 4), (32, 64, 1, 2))


def wino_gemm32_cfg(tile_cfg, wgs=512):
    assert (int(tile_cfg) & 3) < len(WINO_GEMM_TILES32) and 0 <= int(tile_cfg) < 8
    return WINO_GEMM32_CFG0 + int(tile_cfg) + 8 * (int(wgs) // 128)


def is_wino_gemm32_cfg(cfg):
    return WINO_GEMM32_CFG0 <= int(cfg) < PCONV_CFG0


def persistent_cfg_info(cfg):
    """(BM, BN, WM, WN, request depth, workgroups) of a persistent configuration id (>= WINO_GEMM_CFG0)."""
    cfg = int(cfg)
    c = cfg - (PCONV_CFG0 if cfg >= PCONV_CFG0 else WINO_GEMM32_CFG0 if cfg >= WINO_GEMM32_CFG0 else WINO_GEMM_CFG0)
    tiles = WINO_GEMM_TILES32 if is_wino_gemm32_cfg(cfg) else WINO_GEMM_TILES
    return tuple(tiles[c & 3]) + (1 + ((c & 7) >> 2), (c >> 3) * 128)


def wino_gemm_cfg_options(rows_pad, cout, rows32=True):
    """Every persistent configuration that fits a GEMM with ``rows_pad`` rows per component (a 32-row tile only for rows that are a
    multiple of 32; ``rows32=False``: the 64- and 128-row tiles alone -- what the bf16 form of the kernel has)."""
    out = []
    for tc in range(8):
        bm, bn = WINO_GEMM_TILES[tc & 3][:2]
        if rows_pad % bm or (bn > 64 and cout < 128):
            continue
        out += [wino_gemm_cfg(tc, w) for w in (256, 512, 768)]
    for tc in (0, 1, 4, 5) if rows32 else ():
        bm, bn = WINO_GEMM_TILES32[tc & 3][:2]
        if rows_pad % bm or (bn > 64 and cout < 128):
            continue
        out += [wino_gemm32_cfg(tc, w) for w in (256, 512, 768)]
    return out


# ... and from PCONV_CFG0 on: a 1x1 / stride-1 convolution descriptor through the same persistent kernel with the layer's epilogue
# (vfn_conv1x1_persistent_f32), same encoding of tile / request depth / workgroups
PCONV_CFG0 = 2000


def pconv_cfg(tile_cfg, wgs=512):
    return PCONV_CFG0 + int(tile_cfg) + 8 * (int(wgs) // 128)


def pconv_eligible(desc, mode=0):
    """Does vfn_conv1x1_persistent_f32 take this descriptor?  Mirrors every VFN_ERR_ARG condition of that entry point (csrc/
    conv_winograd.hip), so that a descriptor it refuses falls back to the tiled kernels instead of raising at launch."""
    lim = 0x7fffff00
    return (mode == 0 and desc.KH == 1 and desc.KW == 1 and desc.stride == 1 and desc.pad == 0 and not desc.mask and not desc.in_lp and
            not desc.out_lp and not desc.w_packed and not desc.w_batch_rows and desc.Cin % 32 == 0 and desc.in_ld % 4 == 0 and
            desc.M >= 1 and desc.M == desc.N * desc.H * desc.W and desc.M * desc.in_ld * 4 < lim and desc.M * desc.out_ld * 4 < lim and
            desc.cout_pad * desc.Cin * 4 < lim and
            (not desc.res or (desc.res_mod if desc.res_mod > 0 else desc.M) * desc.res_ld * 4 < lim))


def shortcut_fused_eligible(sc, main, mode=0):
    """Does vfn_conv1x1_shortcut_fused_f32 take this pair (shortcut layer, main layer)?  Mirrors every VFN_ERR_ARG condition of that
    entry point (csrc/conv_winograd.hip) but the configuration's filter tile (cout_pad: see shortcut_fused_cfg_options)."""
    lim = 0x7fffff00
    for d in (sc, main):
        if (d.KH != 1 or d.KW != 1 or d.pad != 0 or d.mask or d.in_lp or d.out_lp or d.w_packed or d.ksplit > 1 or d.w_batch_rows or d.res or
                d.Cin < 32 or d.Cin % 32 or d.in_ld < d.Cin or d.in_ld % 4 or d.N < 1 or d.H < 1 or d.W < 1 or not d.inp or not d.w):
            return False
    return (mode == 0 and bool(main.out) and main.stride == 1 and sc.stride in (1, 2) and main.M >= 1 and main.M == main.N * main.H * main.W and
            sc.Ho == (sc.H - 1) // sc.stride + 1 and sc.Wo == (sc.W - 1) // sc.stride + 1 and sc.M == sc.N * sc.Ho * sc.Wo and
            sc.M == main.M and sc.Cout == main.Cout and main.Cout >= 1 and main.out_ld >= main.Cout and
            min(sc.cout_pad, main.cout_pad) >= (main.Cout + 63) // 64 * 64 and
            sc.N * sc.H * sc.W * sc.in_ld * 4 < lim and main.M * main.in_ld * 4 < lim and main.M * main.out_ld * 4 < lim and
            main.cout_pad * main.Cin * 4 < lim and sc.cout_pad * sc.Cin * 4 < lim)


def shortcut_fused_cfg_options(sc, main):
    """(tile cfg 0..3, workgroups) candidates of the fused launch: the persistent kernel's four tiles (operands one K tile ahead) whose
    filter tile both layers' padded filter counts cover."""
    out = []
    for tc in range(4):
        bn = WINO_GEMM_TILES[tc & 3][1]
        if (bn > 64 and main.Cout < 128) or min(sc.cout_pad, main.cout_pad) < (main.Cout + bn - 1) // bn * bn:
            continue
        out += [(tc, w) for w in (256, 512, 768)]
    return out


def shortcut_fused_launch(sc, main, tile_cfg, wgs):
    """The shortcut 1x1 convolution ``sc`` (stride 1 or 2, never written) and the 1x1 convolution ``main`` whose residual it is, as one
    launch of the persistent kernel (include/vfn_shortcut_fused.h)."""
    check(_lib.lib().vfn_conv1x1_shortcut_fused_f32(C.byref(sc), C.byref(main), int(tile_cfg), int(wgs), stream()),
          'vfn_conv1x1_shortcut_fused_f32')


def pconv_cfg_options(cout):
    out = []
    for tc in range(8):
        if WINO_GEMM_TILES[tc & 3][1] > 64 and cout < 128:
            continue
        out += [pconv_cfg(tc, w) for w in (256, 512, 768)]
    return out


# ... and from THIN3X3_CFG0 on: a 3x3 / stride-1 / pad-1 descriptor with 32 filters and 32 or 64 input channels through the LDS-resident
# kernel (vfn_conv3x3_thin_f32, include/vfn_conv_thin.h): id = THIN3X3_CFG0 + 4096 * (Cin == 32) + workgroups of its persistent grid
# (0: one per CU) -- the id names the instantiation, as every other id does
THIN3X3_CFG0 = 3000
THIN3X3_MAX_WGS = _lib.DEFINES_CONV_THIN['VFN_THIN3X3_MAX_WGS']


def thin3x3_cfg(cin, wgs=256):
    assert cin in (32, 64) and 0 <= int(wgs) <= THIN3X3_MAX_WGS < 4096
    return THIN3X3_CFG0 + 4096 * (cin == 32) + int(wgs)


def is_thin3x3_cfg(cfg):
    return THIN3X3_CFG0 <= int(cfg) < THIN3X3_CFG0 + 2 * 4096


def thin3x3_cfg_info(cfg):
    """(Cin, workgroups) of a thin-kernel configuration id."""
    c = int(cfg) - THIN3X3_CFG0
    return (32 if c >= 4096 else 64), c & 4095


def thin3x3_eligible(desc, mode=0, ignore_split=False):
    """Does vfn_conv3x3_thin_f32 take this descriptor?  Mirrors every VFN_ERR_ARG condition of that entry point (csrc/conv_thin3x3.hip).
    ``ignore_split``: would it, once the split-K choice of another kernel is cleared (set_splitk(desc, 1, None): the tuning script)."""
    lim, hw = 0x7fffff00, desc.H * desc.W
    return (mode == 0 and bool(desc.inp) and bool(desc.w) and bool(desc.out) and desc.KH == 3 and desc.KW == 3 and desc.stride == 1 and
            desc.pad == 1 and desc.Cout == 32 and desc.cout_pad >= 32 and desc.Cin in (32, 64) and desc.N >= 1 and desc.H >= 1 and
            desc.W >= 1 and desc.Ho == desc.H and desc.Wo == desc.W and desc.M == desc.N * hw and desc.in_ld >= desc.Cin and
            desc.in_ld % 4 == 0 and desc.out_ld >= 32 and not desc.mask and not desc.in_lp and not desc.out_lp and not desc.w_packed and
            not desc.w_batch_rows and (desc.ksplit <= 1 or ignore_split) and
            (not desc.res or (desc.res_ld >= 32 and desc.res_mod >= 0 and desc.res_mod % hw == 0 and
                              (desc.res_mod if desc.res_mod > 0 else desc.M) * desc.res_ld * 4 < lim)) and
            desc.M * desc.in_ld * 4 < lim and desc.M * desc.out_ld * 4 < lim and (desc.inp | desc.w) % 16 == 0)


def thin3x3_cfg_options(desc):
    """Grids the tuner tries: one workgroup per CU, and two where two fit a CU's LDS (Cin 32)."""
    return [thin3x3_cfg(desc.Cin, w) for w in ((256, 512) if desc.Cin == 32 else (256,))]


def conv2d_launch(desc, cfg, mode=0):
    cfg = int(cfg)
    if is_thin3x3_cfg(cfg):
        if mode != 0:
            raise RuntimeError('the LDS-resident 3x3 convolution is an f32 kernel')
        cin, wgs = thin3x3_cfg_info(cfg)
        if cin != desc.Cin and desc.Cin in (32, 64):
            raise RuntimeError(f'configuration {cfg} names the Cin = {cin} instantiation, the layer has Cin = {desc.Cin}')
        check(_lib.lib().vfn_conv3x3_thin_f32(C.byref(desc), wgs, stream()), 'vfn_conv3x3_thin_f32')
        return
    if cfg >= PCONV_CFG0:
        c = cfg - PCONV_CFG0
        if mode != 0:
            raise RuntimeError('the persistent 1x1 convolution is an f32 kernel')
        check(_lib.lib().vfn_conv1x1_persistent_f32(C.byref(desc), c & 7, (c >> 3) * 128, stream()), 'vfn_conv1x1_persistent_f32')
        return
    if cfg >= WINO_GEMM_CFG0:
        c, rows = cfg - WINO_GEMM_CFG0, desc.w_batch_rows
        if is_wino_gemm32_cfg(cfg):          # a 32-row tile: native configurations 8 .. 15, f32 only
            c = cfg - WINO_GEMM32_CFG0
            if mode != 0 or rows <= 0:
                raise RuntimeError('the 32-row tiles take an f32 Winograd-domain descriptor (w_batch_rows)')
            check(_lib.lib().vfn_winograd_gemm_f32(desc.inp, desc.w, desc.out, desc.M // rows, rows, desc.Cin, desc.Cout, desc.cout_pad,
                                                   8 + (c & 7), (c >> 3) * 128, stream()), 'vfn_winograd_gemm_f32')
            return
        if mode == 1 and rows > 0:           # plain bf16: the descriptor's `inp` / `w` point at bf16 V / bf16 U (make_winograd_gemm_desc on them)
            check(_lib.lib().vfn_winograd_gemm_bf16(desc.inp, desc.w, desc.out, desc.M // rows, rows, desc.Cin, desc.Cout, desc.cout_pad, c & 7,
                                                    (c >> 3) * 128, stream()), 'vfn_winograd_gemm_bf16')
            return
        if mode != 0 or rows <= 0:
            raise RuntimeError('the persistent GEMM takes an f32 (or plain-bf16) Winograd-domain descriptor (w_batch_rows)')
        check(_lib.lib().vfn_winograd_gemm_f32(desc.inp, desc.w, desc.out, desc.M // rows, rows, desc.Cin, desc.Cout, desc.cout_pad, c & 7,
                                               (c >> 3) * 128, stream()), 'vfn_winograd_gemm_f32')
        return
    name = _CONV_FN[int(mode)]
    check(getattr(_lib.lib(), name)(C.byref(desc), cfg, stream()), name)


def conv_cfg_name(cfg, mode=0, _cache={}):
    """Kernel instantiation behind configuration id ``cfg`` as rocprofv3 prints it (conv_cfg_names + the persistent GEMM ids)."""
    cfg = int(cfg)
    if is_thin3x3_cfg(cfg):
        return f'conv_thin3x3_kernel<{thin3x3_cfg_info(cfg)[0]}>'
    if cfg >= WINO_GEMM_CFG0:
        bm, bn, wm, wn, pd, _ = persistent_cfg_info(cfg)
        return f'wino_gemm_kernel<{bm}, {bn}, {wm}, {wn}, {pd}, {"true" if cfg >= PCONV_CFG0 else "false"}, {"true" if mode == 1 else "false"}>'
    if mode not in _cache:
        _cache[mode] = conv_cfg_names(mode)
    return _cache[mode][cfg]


def conv2d_nhwc(x, wp, cout, kh, kw, stride, pad, scale=None, shift=None, res=None,
                relu_in=False, relu_out=False, cfg=3, out=None, mode=0):
    """Convenience form for tests: allocates the output."""
    N, H, W, _ = x.shape
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty(N, Ho, Wo, cout, device=x.device, dtype=torch.float32)
    d = make_conv_desc(x, wp, cout, kh, kw, stride, pad, out, scale, shift, res, relu_in, relu_out)
    if mode == 0 and conv_cfg_kind(cfg) == 2:
        set_streamk(d, *streamk_scratch(x.device))
    conv2d_launch(d, cfg, mode)
    return out


# --------------------------------------------------------------------------- Winograd F(4x4, 3x3)
_WINO_G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                       dtype=torch.float64)
WINO_ROW_MULT = 256                   # rows per transform component are padded to a multiple of the tallest tile
_WINO_KROT = int(os.environ.get('VFN_KROT', '0'))      # vfn_conv_desc.k_rot for the transform-domain GEMMs (0: every workgroup starts at K tile 0)


def pack_winograd_weight(w):
    """[Cout, Cin, 3, 3] conv filters -> U [36 * cout_pad, Cin] f32: U[6i+j] = (G g G^T)[i][j] for every filter pair, computed
    in float64 (the 36 filter banks of the transform-domain GEMMs; cout_pad = Cout rounded up to 256 like pad_rows)."""
    cout, cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3)
    g = w.detach().double().cpu()
    U = torch.einsum('ia,ocab,jb->ijoc', _WINO_G, g, _WINO_G)                 # [6,6,Cout,Cin]
    cp = (cout + 255) // 256 * 256
    out = torch.zeros(36, cp, cin, dtype=torch.float32)
    out[:, :cout] = U.reshape(36, cout, cin).float()
    return out.reshape(36 * cp, cin).contiguous()


def winograd_rows(N, H, W):
    t = N * ((H + 3) // 4) * ((W + 3) // 4)
    return (t + WINO_ROW_MULT - 1) // WINO_ROW_MULT * WINO_ROW_MULT


# Winograd F(6x6, 3x3) (f32 inference layers; csrc/conv_winograd.hip): points 0, +-1, +-2, +-1/2, inf
_WINO6_G = torch.tensor([[1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45], [1 / 90, -1 / 45, 2 / 45],
                         [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=torch.float64)
WINO6_ROW_MULT = 64                   # rows per component are padded to the persistent GEMM's shorter tile (64 x 128, 64 x 64)


def pack_winograd6_weight(w):
    """[Cout, Cin, 3, 3] conv filters -> U [64 * cout_pad, Cin] f32: U[8i+j] = (G g G^T)[i][j] in float64, every product and sum rounded
    on its own in the order of refresh kind 6 (csrc/refresh.hip), so that the device's image of a parameter equals this one bit for bit."""
    cout, cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3)
    g, G = w.detach().double().cpu(), _WINO6_G
    col = lambda k: G[:, k].view(8, 1)
    tmp = (col(0) * g[:, :, None, 0, :] + col(1) * g[:, :, None, 1, :]) + col(2) * g[:, :, None, 2, :]          # G g: [Cout,Cin,8,3]
    U = (tmp[..., 0, None] * G[:, 0] + tmp[..., 1, None] * G[:, 1]) + tmp[..., 2, None] * G[:, 2]               # (G g) G^T: [Cout,Cin,8,8]
    cp = (cout + 255) // 256 * 256
    out = torch.zeros(64, cp, cin, dtype=torch.float32)
    out[:, :cout] = U.permute(2, 3, 0, 1).reshape(64, cout, cin).float()
    return out.reshape(64 * cp, cin).contiguous()


def winograd6_tiles(N, H, W):
    return N * ((H + 5) // 6) * ((W + 5) // 6)


def winograd6_rows(N, H, W):
    return (winograd6_tiles(N, H, W) + WINO6_ROW_MULT - 1) // WINO6_ROW_MULT * WINO6_ROW_MULT


def winograd6_form(N, H, W, C, is_output, has_res):
    """The form of csrc/conv_winograd.hip that an F(6x6) transform call of this shape takes (0: one thread per tile and channel pair,
    2: lane-split; VFN_WINO6_XFORM = 0 / 2 forces one, unset the measured rule)."""
    return _lib.lib().vfn_winograd6_form(N, H, W, C, int(is_output), int(has_res))


def pack_winograd_weight_bf16(w):
    """The 36 transform-domain filter banks (pack_winograd_weight: float64 transform) rounded once to bf16: [36 * cout_pad, Cin] bf16."""
    return pack_winograd_weight(w).to(torch.bfloat16).contiguous()


def winograd_input(x, V, rows_pad, relu, N=None, H=None, W=None, cin=None, ld_x=None, tile=4):
    """``tile`` = 6: the F(6x6, 3x3) transform (V [64 * rows_pad, cin], f32 only)."""
    if N is None:
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
    cin = cin if cin is not None else x.shape[-1]
    ld_x = ld_x if ld_x is not None else x.shape[-1]
    if tile == 6:
        check(_lib.lib().vfn_winograd6_input_f32(ptr(x), N, H, W, cin, ld_x, int(relu), ptr(V), rows_pad, stream()), 'vfn_winograd6_input_f32')
        return
    if V.dtype == torch.bfloat16:            # the plain-bf16 mode: V written as bf16
        check(_lib.lib().vfn_winograd_input_bf16(ptr(x), N, H, W, cin, ld_x, int(relu), ptr(V), rows_pad, stream()), 'vfn_winograd_input_bf16')
        return
    check(_lib.lib().vfn_winograd_input_f32(ptr(x), N, H, W, cin, ld_x, int(relu), ptr(V), rows_pad, stream()), 'vfn_winograd_input_f32')


def winograd_output(Mb, rows_pad, out, N, H, W, cout, scale, shift, res, res_ld, res_mod, relu_out, out_ld=None, tile=4):
    name = 'vfn_winograd6_output_f32' if tile == 6 else 'vfn_winograd_output_f32'
    check(getattr(_lib.lib(), name)(ptr(Mb), rows_pad, N, H, W, cout, ptr(scale), ptr(shift), ptr(res), int(res_ld), int(res_mod),
                                    int(relu_out), ptr(out), out_ld if out_ld is not None else out.shape[-1], stream()), name)


def make_winograd_gemm_desc(V, U, Mb, rows_pad, cin, cout, comps=36):
    """The 36 (F(6x6, 3x3): 64) transform-domain GEMMs as one batched-filter launch of the convolution kernels."""
    d = make_conv_desc(V, U, cout, 1, 1, 1, 0, Mb, None, None, None, False, False, cin=cin, in_ld=cin, out_ld=cout, N=1, H=1, W=comps * rows_pad)
    d.cout_pad = U.shape[0] // comps
    d.w_batch_rows = rows_pad
    d.k_rot = _WINO_KROT
    return d


def winograd_gemm(V, U, Mb, rows_pad, cin, cout, cfg=0, wgs=0, comps=36):
    """The transform-domain GEMMs as one persistent launch (vfn_winograd_gemm_f32): V [comps * rows_pad, cin], U [comps * cout_pad, cin],
    Mb [comps * rows_pad, cout]."""
    check(_lib.lib().vfn_winograd_gemm_f32(ptr(V), ptr(U), ptr(Mb), comps, rows_pad, cin, cout, U.shape[0] // comps, int(cfg), int(wgs), stream()),
          'vfn_winograd_gemm_f32')


def conv2d_winograd(x, w, scale=None, shift=None, res=None, relu_in=False, relu_out=False, cfg=2, res_mod=0, tile=4):
    """Convenience form for tests: x NHWC, w [Cout,Cin,3,3] (torch layout) -> NHWC output of the 3x3 / stride-1 / pad-1 convolution.
    ``tile`` = 6: F(6x6, 3x3) (``cfg``: a persistent configuration whose tile height is 64, or a tiled one)."""
    N, H, W, cin = x.shape
    cout = w.shape[0]
    if tile == 6:
        comps, rows, tiles = 64, winograd6_rows(N, H, W), winograd6_tiles(N, H, W)
        U = pack_winograd6_weight(w).to(x.device)
    else:
        comps, rows, tiles = 36, winograd_rows(N, H, W), vfn_winograd_tiles(N, H, W)
        U = pack_winograd_weight(w).to(x.device)
    V = torch.empty(comps * rows, cin, device=x.device, dtype=torch.float32)
    Mb = torch.empty(comps * rows, cout, device=x.device, dtype=torch.float32)
    out = torch.empty(N, H, W, cout, device=x.device, dtype=torch.float32)
    if rows > tiles and tile != 6:                            # (the F(6x6) input transform zeroes its padding rows itself)
        V.view(comps, rows, cin)[:, tiles:].zero_()
    # (x may be a channel slice of a wider NHWC tensor: the transform walks the pixels at the tensor's own stride)
    assert x.stride(3) == 1 and x.stride(1) == W * x.stride(2) and x.stride(0) == H * x.stride(1)
    winograd_input(x, V, rows, relu_in, ld_x=x.stride(2), tile=tile)
    d = make_winograd_gemm_desc(V, U, Mb, rows, cin, cout, comps)
    if conv_cfg_kind(cfg) == 2:
        set_streamk(d, *streamk_scratch(x.device))
    conv2d_launch(d, cfg, 0)
    winograd_output(Mb, rows, out, N, H, W, cout, scale, shift, res, res.shape[-1] if res is not None else 0, res_mod, relu_out, tile=tile)
    return out


def vfn_winograd_tiles(N, H, W):
    return N * ((H + 3) // 4) * ((W + 3) // 4)


# --------------------------------------------------------------------------- stems / pooling
def make_stem_desc(frame, mask, w, scale, shift, out, mean, std, N, H0, W0, pad, Hp, Wp):
    """frame [3,H0,W0] planar; mask [N,H0,W0] or None; out NHWC [N,Hp/2,Wp/2,64]; pad=(lw,uw,lh,uh)."""
    from ._lib import StemDesc
    d = StemDesc()
    d.frame, d.mask, d.w, d.scale, d.shift, d.out = ptr(frame), ptr(mask), ptr(w), ptr(scale), ptr(shift), ptr(out)
    for i in range(3):
        d.mean[i] = float(mean[i])
        d.std[i] = float(std[i])
    d.N, d.cin = N, (5 if mask is not None else 3)
    d.H0, d.W0 = H0, W0
    d.pad_top, d.pad_left = pad[2], pad[0]
    d.Hp, d.Wp, d.Ho, d.Wo = Hp, Wp, Hp // 2, Wp // 2
    return d


def stem_launch(desc):
    check(_lib.lib().vfn_stem_conv7x7_f32(C.byref(desc), stream()), 'vfn_stem_conv7x7_f32')


def pack_stem_weight(ws):
    """list of [64,c_i,7,7] conv weights -> [sum(c_i)*7*8, 64], k=(plane*7+kh)*8+kw, 8th tap zero."""
    w = torch.cat([x.detach().float() for x in ws], dim=1)          # [64, P, 7, 7]
    P = w.shape[1]
    out = torch.zeros(P, 7, 8, 64, dtype=torch.float32, device=w.device)
    out[:, :, :7, :] = w.permute(1, 2, 3, 0)
    return out.reshape(P * 56, 64).contiguous()


def maxpool3x3s2(x, out):
    N, H, W, Cc = x.shape
    check(_lib.lib().vfn_maxpool3x3s2_nhwc_f32(ptr(x), ptr(out), N, H, W, Cc, stream()), 'vfn_maxpool3x3s2_nhwc_f32')
    return out


# --------------------------------------------------------------------------- decoder pointwise
def upsample2x_add(s, pm, out, s_bcast, out_lp=None, lp_relu=False):
    """out = s + bilinear_x2(pm); ``out_lp``: also the split-bf16 image of (relu of) the result (a bf16x3 conv consumes it)."""
    N, h, w, Cc = out.shape
    if out_lp is not None:
        check(_lib.lib().vfn_upsample2x_add_lp_nhwc_f32(ptr(s), ptr(pm), ptr(out), ptr(out_lp), int(lp_relu), N, h, w, Cc,
                                                        int(s_bcast), stream()), 'vfn_upsample2x_add_lp_nhwc_f32')
        return out
    check(_lib.lib().vfn_upsample2x_add_nhwc_f32(ptr(s), ptr(pm), ptr(out), N, h, w, Cc, int(s_bcast), stream()),
          'vfn_upsample2x_add_nhwc_f32')
    return out


def rough_uncertainty(p, p_up, rough, unc):
    obj_n, h, w, _ = p.shape
    check(_lib.lib().vfn_rough_uncertainty_f32(ptr(p), ptr(p_up), ptr(rough), ptr(unc), obj_n, h, w, stream()),
          'vfn_rough_uncertainty_f32')


def local_stats(r1, rough, hs, hr, hm, lm, conf):
    """AFB_URR.py:226-229.  One fused pass (no scratch) for C = 64 and up to 4 objects; otherwise the two-pass pair, which
    needs the scratch buffers hs [obj,h,w,C], hr / hm [obj,h,w]."""
    obj_n, h, w = rough.shape
    Cc = r1.shape[-1]
    L = _lib.lib()
    if Cc == 64 and obj_n <= 4:
        check(L.vfn_local_stats_f32(ptr(r1), ptr(rough), ptr(lm), ptr(conf), obj_n, h, w, Cc, stream()), 'vfn_local_stats_f32')
        return
    check(L.vfn_local_hpass_f32(ptr(r1), ptr(rough), ptr(hs), ptr(hr), ptr(hm), obj_n, h, w, Cc, stream()),
          'vfn_local_hpass_f32')
    check(L.vfn_local_vpass_f32(ptr(hs), ptr(hr), ptr(hm), ptr(lm), ptr(conf), obj_n, h, w, Cc, stream()),
          'vfn_local_vpass_f32')


def local_stats_two_pass(r1, rough, hs, hr, hm, lm, conf):
    """The unfused pair (tests compare the fused kernel with it)."""
    obj_n, h, w = rough.shape
    Cc = r1.shape[-1]
    L = _lib.lib()
    check(L.vfn_local_hpass_f32(ptr(r1), ptr(rough), ptr(hs), ptr(hr), ptr(hm), obj_n, h, w, Cc, stream()), 'vfn_local_hpass_f32')
    check(L.vfn_local_vpass_f32(ptr(hs), ptr(hr), ptr(hm), ptr(lm), ptr(conf), obj_n, h, w, Cc, stream()), 'vfn_local_vpass_f32')


def pred2_gather(z, bias, out):
    """z [N,h,w,ldz] (tap GEMM output) -> out [N,h,w,2] = bias + sum of the nine shifted taps."""
    N, h, w, ldz = z.shape
    check(_lib.lib().vfn_pred2_gather_f32(ptr(z), ptr(bias), ptr(out), N, h, w, ldz, stream()), 'vfn_pred2_gather_f32')
    return out


def final_logits(p_up, unc, conf, q, score, pad, H0, W0):
    obj_n, h, w, _ = p_up.shape
    check(_lib.lib().vfn_final_logits_f32(ptr(p_up), ptr(unc), ptr(conf), ptr(q), ptr(score), obj_n, h, w,
                                          pad[2], pad[0], H0, W0, stream()), 'vfn_final_logits_f32')


def segment_uncertainty(score):
    """score: logits [bs,obj,H,W] from segment -> 0-dim tensor (AFB_URR.py:302-305)."""
    bs, obj_n, H, W = score.shape
    assert score.is_contiguous()
    partial = torch.empty(bs * 64, device=score.device, dtype=torch.float32)
    out = torch.empty(1, device=score.device, dtype=torch.float32)
    check(_lib.lib().vfn_segment_uncertainty_f32(ptr(score), bs, obj_n, H * W, ptr(partial), ptr(out), stream()),
          'vfn_segment_uncertainty_f32')
    return out[0]


def segment_loss(score, label, lu, want_grad=True):
    """train_video_seg.py:72-74 on the logits ``segment`` returns: score f32 [bs,obj,H,W], label int [bs,H,W] ->
    (stats f32[3+bs] = loss, cross entropy, uncertainty, ||u|| per sample; dloss/dscore [bs,obj,H,W] or None)."""
    bs, obj_n, H, W = score.shape
    assert score.is_contiguous()
    lab = label.to(device=score.device, dtype=torch.int32).contiguous()
    partial = torch.empty(2 * bs * 64, device=score.device, dtype=torch.float32)
    stats = torch.empty(3 + bs, device=score.device, dtype=torch.float32)
    grad = torch.empty_like(score) if want_grad else None
    check(_lib.lib().vfn_segment_loss_f32(ptr(score), ptr(lab), bs, obj_n, H * W, float(lu), ptr(partial), ptr(stats), ptr(grad),
                                          stream()), 'vfn_segment_loss_f32')
    return stats, grad


_wgrad_ws = {}
# 1: the pixel slices of a weight gradient are finished inside the launch (vfn_wgrad_desc.tile_counters).  Measured SLOWER on the training
# step (49.6 against 43.1 ms: the wave that arrives last walks ksplit x 64 dwords alone, where the reduce launch spreads them over
# the chip), so it is off; tests/test_kernels_gpu.py keeps the path correct.
_WGRAD_INLAUNCH = os.environ.get('VFN_WGRAD_INLAUNCH', '0') == '1'
_STEM_WGRAD = os.environ.get('VFN_STEM_WGRAD', '1') == '1'        # the 7x7 stems' weight gradient through vfn_stem_wgrad_f32 (0: the generic kernel)


def conv_wgrad(x, gy, k, stride, pad, cin=None, cout=None, ld_x=None, relu=False, rowscale=None, out=None, accumulate=False,
               N=None, H=None, W=None, ksplit=None, batch=1, x_bstride=0, g_bstride=0):
    """dL/dW of y = conv_{k x k, stride, pad}(act(x)) as an implicit GEMM over the pixels (vfn_conv_wgrad_f32): x NHWC
    [N,H,W,ld_x] (``cin`` channels used), gy [N,Ho,Wo,ld_g] (``cout`` used) -> out [cout, k*k*cin] in the packed filter layout
    (kh, kw, cin); ``rowscale`` [cout]: the frozen BatchNorm scale; ``accumulate``: add to ``out``."""
    from ._lib import WgradDesc
    if N is None:
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
    Ho, Wo = gy.shape[1], gy.shape[2]
    ld_x = ld_x if ld_x is not None else (x.stride(-2) if x.dim() >= 2 else x.shape[-1])     # (channel-sliced views keep their pixel stride)
    cin = cin if cin is not None else x.shape[-1]
    cout = cout if cout is not None else gy.shape[-1]
    ld_g = gy.stride(-2)
    assert x.stride(-1) == 1 and gy.stride(-1) == 1
    Kc = k * k * cin
    if out is None:
        assert not accumulate
        out = torch.empty(cout, Kc, device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == batch * cout * Kc
    M = N * Ho * Wo
    if (_STEM_WGRAD and k == 7 and stride == 2 and pad == 3 and cout == 64 and cin in (3, 5) and ld_x == cin and ld_g == 64 and batch == 1
            and not relu and ksplit is None and Ho == (H - 1) // 2 + 1 and Wo == (W - 1) // 2 + 1):
        # the encoders' stems: the operand columns are (kw, c) of one filter row, one pixel walk for all 49 taps (vfn_stem_wgrad_f32)
        L = _lib.lib()
        key = (str(x.device), torch.cuda.current_stream(x.device).cuda_stream, 'stem')
        need = L.vfn_stem_wgrad_scratch_floats(cin)
        part = _wgrad_ws.get(key)
        if part is None or part.numel() < need:
            part = _wgrad_ws[key] = torch.empty(need, device=x.device, dtype=torch.float32)
        check(L.vfn_stem_wgrad_f32(ptr(x), ptr(gy), ptr(rowscale), ptr(out), ptr(part), part.numel(), N, H, W, cin, Ho, Wo, int(accumulate),
                                   stream()), 'vfn_stem_wgrad_f32')
        return out
    tiles = ((cout + 63) // 64 if cout > 32 else 1) * k * k * ((cin + (31 if cin <= 32 else 63)) // (32 if cin <= 32 else 64))
    tiles *= batch                               # (``batch`` independent problems of this shape in one launch: vfn_wgrad_desc.batch)
    if ksplit is None:
        # ~2 000 workgroups, at least 300 pixels per slice (swept on the training step's 51 shapes, scripts/bench_wgrad_shapes.py:
        # 20.0 -> 17.5 ms per step against the first rule, 17.3 with the best split of every shape)
        ksplit = max(1, min(64, 2048 // tiles, M // 300))
        if batch == 1 and cin > 32:
            # round 5 (the step's launches are five times fewer and larger since the decoder is batched over a sample's frames): the
            # 1x1 / 3x3 layers with 3 000 ... 50 000 pixels are fastest with at least 256 workgroups and about 800 pixels per slice --
            # 12 500 x 256 x 512: 71 -> 56 us, 3 125 x 1024 x 256: 40 -> 35 (profiles/r05_wgrad_shapes.txt); the 7x7 stems and the
            # Winograd-domain batches keep the rule above
            ksplit = max(1, min(64, M // 300, max((256 + tiles - 1) // tiles, M // 800)))
    d = WgradDesc()
    d.x, d.gy, d.rowscale, d.dw = ptr(x), ptr(gy), ptr(rowscale), ptr(out)
    d.N, d.H, d.W, d.Cin, d.ld_x = N, H, W, cin, ld_x
    d.Ho, d.Wo, d.Cout, d.ld_g = Ho, Wo, cout, ld_g
    d.k, d.stride, d.pad, d.relu, d.accumulate, d.ksplit = k, stride, pad, int(relu), int(accumulate), int(ksplit)
    d.batch, d.x_bstride, d.g_bstride = int(batch), int(x_bstride), int(g_bstride)
    part = None
    if ksplit > 1:
        key = (str(x.device), torch.cuda.current_stream(x.device).cuda_stream)     # (a workspace per stream: the backward pass
        need = batch * ksplit * cout * Kc                                               #  runs weight gradients beside the data-gradient chain)
        hit = _wgrad_ws.get(key)
        if hit is None or hit[0].numel() < need:
            # (+ the tiles' arrival counters of the in-launch finish, zero at rest; VFN_WGRAD_INLAUNCH=0: the separate reduce launch)
            hit = (torch.empty(max(need, 8 * 1024 * 1024), device=x.device, dtype=torch.float32),
                   hit[1] if hit is not None else torch.zeros(16384, dtype=torch.int32, device=x.device))
            _wgrad_ws[key] = hit
        part = hit[0]
        if _WGRAD_INLAUNCH and tiles <= hit[1].numel() and need * 4 < 0x7fffff00:
            d.tile_counters = ptr(hit[1])
    d.partial = ptr(part)
    check(_lib.lib().vfn_conv_wgrad_f32(C.byref(d), stream()), 'vfn_conv_wgrad_f32')
    return out


def winograd_gy(gy, Z, rows_pad, N, H, W, cout, ld_g):
    check(_lib.lib().vfn_winograd_gy_f32(ptr(gy), N, H, W, cout, ld_g, ptr(Z), rows_pad, stream()), 'vfn_winograd_gy_f32')


_wino_wgrad_ws = {}


def conv_wgrad_winograd(x, gy, cin=None, cout=None, ld_x=None, relu=False, rowscale=None, out=None, accumulate=False, N=None, H=None, W=None):
    """dL/dW of a 3x3 / stride-1 / pad-1 convolution in the Winograd domain (csrc/conv_winograd.hip: dW = G^T [sum_tiles (B^T d B)
    (.) (A dY A^T)] G, a quarter of the direct form's multiplies): input transform of act(x), transform of the gradient tiles,
    the 36 component sums as ONE batched launch of the weight-gradient kernel, back-transform with the row scale / accumulation.
    Same arguments and packed result [cout, 9 * cin] as ``conv_wgrad``; scratch per stream."""
    if N is None:
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
    ld_x = ld_x if ld_x is not None else x.stride(-2)
    cin = cin if cin is not None else x.shape[-1]
    cout = cout if cout is not None else gy.shape[-1]
    ld_g = gy.stride(-2)
    assert cin % 4 == 0 and cout % 4 == 0 and x.stride(-1) == 1 and gy.stride(-1) == 1
    if out is None:
        assert not accumulate
        out = torch.empty(cout, 9 * cin, device=x.device, dtype=torch.float32)
    tiles = vfn_winograd_tiles(N, H, W)
    rows = winograd_rows(N, H, W)
    key = (str(x.device), torch.cuda.current_stream(x.device).cuda_stream)
    need = (36 * rows * cin, 36 * rows * cout, 36 * cout * cin)
    ws = _wino_wgrad_ws.get(key)
    if ws is None or any(t.numel() < n_ for t, n_ in zip(ws, need)):
        old = ws or (None, None, None)
        ws = tuple(t if (t is not None and t.numel() >= n_) else torch.empty(n_, device=x.device, dtype=torch.float32) for t, n_ in zip(old, need))
        _wino_wgrad_ws[key] = ws
    V, Z, dU = ws[0][:need[0]], ws[1][:need[1]], ws[2][:need[2]]
    winograd_input(x, V, rows, relu, N, H, W, cin, ld_x)
    winograd_gy(gy, Z, rows, N, H, W, cout, ld_g)
    # component 0's rows as a one-row image of ``tiles`` pixels; the other 35 components follow at the batch strides
    conv_wgrad(V[:tiles * cin].view(1, 1, tiles, cin), Z[:tiles * cout].view(1, 1, tiles, cout), 1, 1, 0, cin=cin, cout=cout, ld_x=cin,
               out=dU.view(36 * cout, cin), N=1, H=1, W=tiles, batch=36, x_bstride=rows * cin, g_bstride=rows * cout)
    check(_lib.lib().vfn_winograd_dw_f32(ptr(dU), cout, cin, ptr(rowscale), ptr(out), int(accumulate), stream()), 'vfn_winograd_dw_f32')
    return out


def segment_uncertainty_backward(score, g_unc, g_score=None):
    """dL/dscores [bs,obj,H,W] = g_score (optional, from the caller's criterion) + g_unc * d uncertainty / d scores, where
    ``g_unc`` is dL/duncertainty as a 0-dim DEVICE tensor (autograd's hand-over; no host synchronisation)."""
    bs, obj_n, H, W = score.shape
    assert score.is_contiguous() and g_unc.is_cuda and g_unc.numel() == 1 and g_unc.dtype == torch.float32
    if g_score is not None:
        g_score = g_score.to(torch.float32).contiguous()
        assert g_score.shape == score.shape
    partial = torch.empty(2 * bs * 64, device=score.device, dtype=torch.float32)
    stats = torch.empty(3 + bs, device=score.device, dtype=torch.float32)
    grad = torch.empty_like(score)
    check(_lib.lib().vfn_segment_uncertainty_backward_f32(ptr(score), bs, obj_n, H * W, ptr(g_unc), ptr(g_score), ptr(partial),
                                                          ptr(stats), ptr(grad), stream()), 'vfn_segment_uncertainty_backward_f32')
    return grad


# --------------------------------------------------------------------------- loop operators
def resize_bicubic(x, Ho, Wo, out=None):
    """x [C,Hi,Wi] (or [1,C,Hi,Wi]) float32 -> [.., Ho, Wo]."""
    shp = x.shape
    Cc, Hi, Wi = shp[-3], shp[-2], shp[-1]
    assert x.is_contiguous() and x.numel() == Cc * Hi * Wi
    if out is None:
        out = torch.empty(*shp[:-2], Ho, Wo, device=x.device, dtype=torch.float32)
    check(_lib.lib().vfn_resize_bicubic_f32(ptr(x), ptr(out), Cc, Hi, Wi, Ho, Wo, stream()), 'vfn_resize_bicubic_f32')
    return out


def resize_nearest(x, Ho, Wo, out=None):
    shp = x.shape
    Cc, Hi, Wi = shp[-3], shp[-2], shp[-1]
    assert x.is_contiguous() and x.numel() == Cc * Hi * Wi
    if out is None:
        out = torch.empty(*shp[:-2], Ho, Wo, device=x.device, dtype=torch.float32)
    check(_lib.lib().vfn_resize_nearest_f32(ptr(x), ptr(out), Cc, Hi, Wi, Ho, Wo, stream()), 'vfn_resize_nearest_f32')
    return out


def softmax_objects(score, out=None):
    """score [1,obj,H,W] -> softmax over dim 1."""
    obj_n = score.shape[-3]
    n = score.shape[-2] * score.shape[-1]
    assert score.is_contiguous()
    if out is None:
        out = torch.empty_like(score)
    check(_lib.lib().vfn_softmax_objects_f32(ptr(score), ptr(out), obj_n, n, stream()), 'vfn_softmax_objects_f32')
    return out


def resize_argmax(prob, Ho, Wo, out=None):
    """prob [1,obj,Hi,Wi] -> uint8 labels [Ho,Wo] = argmax over objects of the bicubic-resized maps."""
    obj_n, Hi, Wi = prob.shape[-3], prob.shape[-2], prob.shape[-1]
    assert prob.is_contiguous()
    if out is None:
        out = torch.empty(Ho, Wo, device=prob.device, dtype=torch.uint8)
    check(_lib.lib().vfn_resize_argmax_u8(ptr(prob), ptr(out), obj_n, Hi, Wi, Ho, Wo, stream()), 'vfn_resize_argmax_u8')
    return out


def postprocess_pred(pred_np):
    """Host uint8 [H,W] -> uint8 [H,W] (largest 8-connected water blob; myutils/data.py:17-37)."""
    import numpy as np
    pred_np = np.ascontiguousarray(pred_np, dtype=np.uint8)
    out = np.empty_like(pred_np)
    H, W = pred_np.shape
    check(_lib.lib().vfn_postprocess_pred_u8(pred_np.ctypes.data_as(C.c_void_p), H, W,
                                             out.ctypes.data_as(C.c_void_p)), 'vfn_postprocess_pred_u8')
    return out


def postprocess_pred_device(label, out=None, scratch=None):
    """Device uint8 [H,W] -> uint8 [H,W]: postprocessing_pred on the GPU (union-find CCL, largest blob)."""
    H, W = label.shape
    if out is None:
        out = torch.empty_like(label)
    if scratch is None:
        scratch = torch.empty(2 * H * W + 8, dtype=torch.int32, device=label.device)
    check(_lib.lib().vfn_postprocess_pred_device_u8(ptr(label), ptr(out), ptr(scratch), H, W, stream()),
          'vfn_postprocess_pred_device_u8')
    return out


def to_tensor_device(img_u8, out=None):
    """torchvision ToTensor on the device: uint8 [H,W,3] (device) -> float32 [3,H,W] = x / 255."""
    H, W, c = img_u8.shape
    assert c == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous()
    if out is None:
        out = torch.empty(3, H, W, device=img_u8.device, dtype=torch.float32)
    check(_lib.lib().vfn_to_tensor_u8(ptr(img_u8), ptr(out), H, W, stream()), 'vfn_to_tensor_u8')
    return out


_palette_cache = {}


def overlay_device(frame, label, palette, alpha=0.4, cscale=1, out=None):
    """add_overlay + save_overlay's uint8 conversion on the device (myutils/data.py:56-84).
    frame f32 [3,H,W] in [0,1], label uint8 [H,W] (both on the GPU); returns RGB uint8 [H,W,3] on the GPU."""
    _, H, W = frame.shape
    key = (tuple(palette), frame.device)
    if key not in _palette_cache:
        pal = (list(palette) + [0] * 768)[:768]
        _palette_cache[key] = (torch.tensor(pal, dtype=torch.uint8, device=frame.device),
                               torch.empty(1, dtype=torch.int32, device=frame.device))
    pal, scratch = _palette_cache[key]
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=frame.device)
    check(_lib.lib().vfn_overlay_u8(ptr(frame), ptr(label), ptr(pal), ptr(scratch), ptr(out), H, W,
                                    float(alpha), float(cscale), stream()), 'vfn_overlay_u8')
    return out


# --------------------------------------------------------------------------- bank
def row_norms(x, stride_obj, ld, dim, len_dev, rows, obj_n, nrm, inv, stride_n):
    check(_lib.lib().vfn_row_norms(ptr(x), int(stride_obj), ld, dim, ptr(len_dev), rows, obj_n, ptr(nrm), ptr(inv),
                                   int(stride_n), stream()), 'vfn_row_norms')


def scatter_mean_checked_launch(src, index, index_s0, out, status):
    """src [D,S] (any strides), index int64 (row 0 contiguous; ``index_s0`` = row stride of a materialised [D,S] index, 0 for
    a broadcast / 1-D one), out [D,B] (any strides), status int32[1] on the device (sticky: bit 0 = a target outside
    [0, B), bit 1 = index rows differ).  No host synchronisation."""
    D, S = src.shape
    check(_lib.lib().vfn_scatter_mean_checked_f32(ptr(src), src.stride(0), src.stride(1), ptr(index), int(index_s0), S, ptr(out),
                                                  out.stride(0), out.stride(1), D, out.shape[1], ptr(status), stream()),
          'vfn_scatter_mean_checked_f32')


def scatter_mean_launch(src, index_row, out):
    """src [D,S] (any strides), index_row int64 [S] contiguous, out [D,B] (any strides)."""
    D, S = src.shape
    check(_lib.lib().vfn_scatter_mean_f32(ptr(src), src.stride(0), src.stride(1), ptr(index_row), S, ptr(out),
                                          out.stride(0), out.stride(1), D, stream()), 'vfn_scatter_mean_f32')


# --------------------------------------------------------------------------- water level by reference object
def _host_ints(values, cols, what):
    """(ctypes int array, R) of an [R][cols] table of host integers."""
    import numpy as np
    a = np.asarray(values)
    if a.ndim != 2 or a.shape[1] != cols or a.shape[0] < 1 or a.dtype.kind not in 'iu':
        raise ValueError(f'{what}: expected integers [R][{cols}] with R >= 1, got {a.dtype} {a.shape}')
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a.ctypes.data_as(C.POINTER(C.c_int)), a.shape[0], a


def inverse_homography(homo_mat):
    """The 9 doubles vfn_warp_perspective_* take: ``numpy.linalg.inv`` of the source -> destination matrix in float64
    (what cv2.warpPerspective does inside without WARP_INVERSE_MAP)."""
    import numpy as np
    m = np.asarray(homo_mat, dtype=np.float64)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError(f'homography: expected a finite 3 x 3 matrix, got shape {m.shape}')
    inv = np.ascontiguousarray(np.linalg.inv(m), dtype=np.float64).reshape(9)
    if not np.isfinite(inv).all():
        raise ValueError('homography: the matrix has no finite inverse')
    return inv


def warp_perspective_u8(img, homo_mat, out=None, inverse=None):
    """cv2.warpPerspective(img, homo_mat, (W, H)) with default flags on the device (include/vfn_hip.h states the arithmetic).
    ``img``: uint8 [H,W] or [H,W,C] with C = 1 / 3, or the loop's frame float32 [3,H,W] in [0,1] (every sample is made uint8
    by truncation of x * 255 before it is interpolated; the result is float32 [3,H,W] = byte / 255, what ``overlay_device``
    takes).  ``inverse``: the 9 doubles of ``inverse_homography(homo_mat)`` when the caller keeps them."""
    _lib.require_gpu(img, 'warp_perspective_u8: img')
    inv = inverse_homography(homo_mat) if inverse is None else inverse
    minv = inv.ctypes.data_as(C.POINTER(C.c_double))
    if not img.is_contiguous():
        raise ValueError('warp_perspective_u8: img must be contiguous')
    if out is None:
        out = torch.empty_like(img)
    if out.shape != img.shape or out.dtype != img.dtype or not out.is_contiguous() or out.data_ptr() == img.data_ptr():
        raise ValueError('warp_perspective_u8: out must be another contiguous tensor of the shape and type of img')
    if img.dtype == torch.float32 and img.dim() == 3 and img.shape[0] == 3:
        _, H, W = img.shape
        check(_lib.lib().vfn_warp_perspective_f32(ptr(img), ptr(out), H, W, minv, stream()), 'vfn_warp_perspective_f32')
    elif img.dtype == torch.uint8 and (img.dim() == 2 or (img.dim() == 3 and img.shape[2] in (1, 3))):
        H, W = img.shape[:2]
        check(_lib.lib().vfn_warp_perspective_u8(ptr(img), ptr(out), H, W, 1 if img.dim() == 2 else img.shape[2], minv, stream()),
              'vfn_warp_perspective_u8')
    else:
        raise ValueError(f'warp_perspective_u8: uint8 [H,W] / [H,W,1] / [H,W,3] or float32 [3,H,W], got {img.dtype} {tuple(img.shape)}')
    return out


def _log_args(log, t, R, what):
    if not (log.is_cuda and log.dtype == torch.int32 and log.dim() == 2 and log.is_contiguous() and log.shape[1] == R):
        raise ValueError(f'{what}: log must be a contiguous int32 [T][{R}] tensor on the GPU')
    if not 0 <= int(t) < log.shape[0]:
        raise ValueError(f'{what}: row {t} outside a log of {log.shape[0]} rows')


def waterline_scan(label, keypoints, log, t, water_label=1):
    """Row ``t`` of the device log int32 [T,R] := per key point (kx, ky) (host integers [R][2]) the offset row - ky of the first
    row below it whose label is ``water_label``, or -1 (reference_tracking.py:197-204).  A key point outside the image raises
    ``ValueError`` (the reference: IndexError).  No host synchronisation."""
    _lib.require_gpu(label, 'waterline_scan: label')
    if label.dtype != torch.uint8 or label.dim() != 2 or not label.is_contiguous():
        raise ValueError('waterline_scan: label must be a contiguous uint8 [H,W] tensor')
    H, W = label.shape
    kp, R, a = _host_ints(keypoints, 2, 'waterline_scan: keypoints')
    _log_args(log, t, R, 'waterline_scan')
    if ((a[:, 0] < 0) | (a[:, 0] >= W) | (a[:, 1] < 0) | (a[:, 1] >= H)).any():
        raise ValueError(f'waterline_scan: key point outside the {W} x {H} image: {a.tolist()}')
    check(_lib.lib().vfn_waterline_scan(ptr(label), H, W, kp, R, int(water_label), ptr(log), log.shape[0], int(t), stream()),
          'vfn_waterline_scan')
    return log


def waterlevel_draw(overlay, boxes, log, t):
    """In place on the RGB uint8 [H,W,3] overlay: the reference boxes (host integers [R][4] = x, y, w, h) in green and, where row
    ``t`` of the device log holds an offset d > 1, the line from the key point down to the water in red (the rule is stated
    in include/vfn_hip.h).  The log is read on the device."""
    _lib.require_gpu(overlay, 'waterlevel_draw: overlay')
    if overlay.dtype != torch.uint8 or overlay.dim() != 3 or overlay.shape[2] != 3 or not overlay.is_contiguous():
        raise ValueError('waterlevel_draw: overlay must be a contiguous uint8 [H,W,3] tensor')
    H, W, _ = overlay.shape
    bx, R, a = _host_ints(boxes, 4, 'waterlevel_draw: boxes')
    _log_args(log, t, R, 'waterlevel_draw')
    if (a[:, 2:] < 0).any() or (abs(a) > 1 << 24).any():
        raise ValueError(f'waterlevel_draw: boxes must have w, h >= 0 and image-sized coordinates: {a.tolist()}')
    check(_lib.lib().vfn_waterlevel_draw_u8(ptr(overlay), H, W, bx, R, ptr(log), log.shape[0], int(t), stream()),
          'vfn_waterlevel_draw_u8')
    return overlay


# --------------------------------------------------------------------------- reference boxes followed through the clip
TRACK_MAX_SIDE, TRACK_MAX_RADIUS = _lib.DEFINES['VFN_TRACK_MAX_SIDE'], _lib.DEFINES['VFN_TRACK_MAX_RADIUS']


def track_luma(frame, out=None):
    """The tracker's luma uint8 [H,W] of the loop's frame float32 [3,H,W] in [0,1] (include/vfn_hip.h states the arithmetic)."""
    _lib.require_gpu(frame, 'track_luma: frame')
    if frame.dtype != torch.float32 or frame.dim() != 3 or frame.shape[0] != 3 or not frame.is_contiguous():
        raise ValueError(f'track_luma: frame must be a contiguous float32 [3,H,W] tensor, got {frame.dtype} {tuple(frame.shape)}')
    _, H, W = frame.shape
    if out is None:
        out = torch.empty(H, W, dtype=torch.uint8, device=frame.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W) or not out.is_contiguous() or out.device != frame.device:
        raise ValueError('track_luma: out must be a contiguous uint8 [H,W] tensor beside the frame')
    check(_lib.lib().vfn_track_luma_f32(ptr(frame), ptr(out), H, W, stream()), 'vfn_track_luma_f32')
    return out


class TrackState:
    """What the tracker keeps on the device between two frames: ``box`` int32 [R,4], ``t16`` the templates uint16 (8.8 fixed
    point, reference r's [h,w] at ``offsets[r]``) and ``acc``, the search's sums (zero between two updates)."""

    def __init__(self, boxes, radius, device):
        import numpy as np
        self.radius = int(radius)
        self.R = boxes.shape[0]
        self.sizes = np.ascontiguousarray(boxes[:, 2:], dtype=np.int32)
        area = self.sizes[:, 0].astype(np.int64) * self.sizes[:, 1]
        self.offsets = [int(v) for v in np.concatenate([[0], np.cumsum(area)])]
        self.box = torch.zeros(self.R, 4, dtype=torch.int32, device=device)
        self.t16 = torch.zeros(max(1, self.offsets[-1]), dtype=torch.int16, device=device)         # (the bits of a uint16)
        self.acc = torch.zeros(self.R * (2 * self.radius + 1) ** 2 * 3, dtype=torch.int64, device=device)

    def template(self, r):
        """Reference r's template as int64 [h,w] on the host (one D2H; for tests and inspection)."""
        w, h = (int(v) for v in self.sizes[r])
        return (self.t16[self.offsets[r]:self.offsets[r + 1]].cpu().numpy().view('uint16').astype('int64')).reshape(h, w)


def _luma_args(luma, what):
    _lib.require_gpu(luma, f'{what}: luma')
    if luma.dtype != torch.uint8 or luma.dim() != 2 or not luma.is_contiguous():
        raise ValueError(f'{what}: luma must be a contiguous uint8 [H,W] tensor')
    return luma.shape


def track_init(luma, boxes, radius=16):
    """A ``TrackState`` for the reference boxes (host integers [R][4] = x, y, w, h, inside the image, sides 1 ..
    ``TRACK_MAX_SIDE``) with the templates cut out of ``luma``; ``radius``: the search radius, 1 .. ``TRACK_MAX_RADIUS``."""
    H, W = _luma_args(luma, 'track_init')
    bx, R, a = _host_ints(boxes, 4, 'track_init: boxes')
    if not 1 <= int(radius) <= TRACK_MAX_RADIUS:
        raise ValueError(f'track_init: search radius {radius} outside 1 .. {TRACK_MAX_RADIUS}')
    if R > 32 or (a[:, 2:] < 1).any() or (a[:, 2:] > TRACK_MAX_SIDE).any():
        raise ValueError(f'track_init: at most 32 boxes with sides 1 .. {TRACK_MAX_SIDE}: {a.tolist()}')
    if (a[:, :2] < 0).any() or (a[:, 0] + a[:, 2] > W).any() or (a[:, 1] + a[:, 3] > H).any():
        raise ValueError(f'track_init: box outside the {W} x {H} image: {a.tolist()}')
    st = TrackState(a, radius, luma.device)
    check(_lib.lib().vfn_track_init(ptr(luma), H, W, bx, R, st.radius, ptr(st.box), ptr(st.t16), st.t16.numel(), ptr(st.acc),
                                    st.acc.numel(), stream()), 'vfn_track_init')
    return st


def track_update(state, luma, box_log, ok_log, score_log, t):
    """One frame of the tracker for all references of ``state``: search, arg-max, failure test, box move and template update on
    the device; row ``t`` of ``box_log`` int32 [T,R,4], ``ok_log`` int32 [T,R] and ``score_log`` float32 [T,R] is written.  No host
    synchronisation."""
    H, W = _luma_args(luma, 'track_update')
    R = state.R
    T = box_log.shape[0]
    for log, dt, shape, what in ((box_log, torch.int32, (T, R, 4), 'box_log'), (ok_log, torch.int32, (T, R), 'ok_log'),
                                 (score_log, torch.float32, (T, R), 'score_log')):
        if not (log.is_cuda and log.dtype == dt and tuple(log.shape) == shape and log.is_contiguous()):
            raise ValueError(f'track_update: {what} must be a contiguous {dt} tensor of shape {shape} on the GPU')
    if not 0 <= int(t) < T:
        raise ValueError(f'track_update: row {t} outside logs of {T} rows')
    check(_lib.lib().vfn_track_update(ptr(luma), H, W, state.sizes.ctypes.data_as(C.POINTER(C.c_int)), R, state.radius, ptr(state.box),
                                      ptr(state.t16), state.t16.numel(), ptr(state.acc), state.acc.numel(), ptr(box_log), ptr(ok_log),
                                      ptr(score_log), T, int(t), stream()), 'vfn_track_update')


def _dev_boxes(boxes, what):
    if not (boxes.is_cuda and boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 4 and boxes.shape[0] >= 1
            and boxes.is_contiguous()):
        raise ValueError(f'{what}: boxes must be a contiguous int32 [R,4] tensor on the GPU')
    return boxes.shape[0]


def waterline_scan_dev(label, boxes, log, t, water_label=1):
    """``waterline_scan`` under boxes int32 [R,4] = (x, y, w, h) that live on the device (a row of the tracker's box log): the key
    point (int(x + w / 2), y + h) is computed there, and one without a row of the image below it logs -1."""
    _lib.require_gpu(label, 'waterline_scan_dev: label')
    if label.dtype != torch.uint8 or label.dim() != 2 or not label.is_contiguous():
        raise ValueError('waterline_scan_dev: label must be a contiguous uint8 [H,W] tensor')
    H, W = label.shape
    R = _dev_boxes(boxes, 'waterline_scan_dev')
    _log_args(log, t, R, 'waterline_scan_dev')
    check(_lib.lib().vfn_waterline_scan_dev(ptr(label), H, W, ptr(boxes), R, int(water_label), ptr(log), log.shape[0], int(t), stream()),
          'vfn_waterline_scan_dev')
    return log


def waterlevel_draw_dev(overlay, boxes, log, t):
    """``waterlevel_draw`` under boxes int32 [R,4] that live on the device."""
    _lib.require_gpu(overlay, 'waterlevel_draw_dev: overlay')
    if overlay.dtype != torch.uint8 or overlay.dim() != 3 or overlay.shape[2] != 3 or not overlay.is_contiguous():
        raise ValueError('waterlevel_draw_dev: overlay must be a contiguous uint8 [H,W,3] tensor')
    H, W, _ = overlay.shape
    R = _dev_boxes(boxes, 'waterlevel_draw_dev')
    _log_args(log, t, R, 'waterlevel_draw_dev')
    check(_lib.lib().vfn_waterlevel_draw_dev(ptr(overlay), H, W, ptr(boxes), R, ptr(log), log.shape[0], int(t), stream()),
          'vfn_waterlevel_draw_dev')
    return overlay
