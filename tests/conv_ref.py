"""Float64 reference, case lists and buffer layout of the convolution kernel tests (tests/test_conv_kernels_gpu.py, checked on the
CPU by tests/test_conv_ref_host.py).

Reference: float64 ``F.conv2d`` and the epilogue of vfn_conv_desc written ONCE (``epilogue``); for the reduced-precision modes the
float64 evaluation of exactly the products the kernels form (``reduced_reference``).  Bound: the reference's own float32 error --
``ratio`` = the larger of float32 ``F.conv2d`` and a float32 running sum in the kernels' K order (kh, kw, cin), both against float64
in units of max|ref|; a kernel may be ``FACTOR`` x ratio away, and a case whose bound is not below ``BOUND_CAP`` is refused.
Layout (``Layout``): every tensor is a channel slice of a wider allocation with whole guard rows before and after it; gutters and
guard rows are poisoned, so a read or a write outside a tensor shows in the result or in the bytes around it."""
import functools

import torch
from torch.nn import functional as F

FACTOR = 8.0            # the factor the other kernel test files allow over the reference's own float32 error
BOUND_CAP = 2e-5        # ten times tighter than the 2e-4 of tests/test_conv_gpu.py
# Floor of ``ratio``: one rounding to float32 of a value of size max|ref|.  The two 4-output geometries have so few outputs that a
# float32 evaluation lands on the float64 value by luck (measured ratios down to 1.3e-8, a fifth of a rounding), which says nothing
# about another summation order; no float32 result is defined more finely than its own rounding.
RATIO_FLOOR = 2.0 ** -24
NAN = float('nan')
BIG = 1.0e30            # poison under a ReLU: fmaxf drops a NaN, a finite value that wrecks the bound survives it
GUARD = 3               # whole guard rows before and after every tensor

# (N, H, W, Cin, Cout, k, stride): the smallest shapes that reach each edge
GEOMS = (
    (1, 1, 1, 32, 4, 1, 1),         # M = 1, one K tile: fewer than the K groups / the prefetch depth, odd under two tiles per barrier
    (1, 1, 1, 32, 4, 3, 1),         # 8 of 9 taps outside the image
    (2, 5, 7, 32, 36, 3, 1),        # every pixel on the border, M = 70 ragged for every tile height, Cout = one 32-filter tile + 4
    (1, 13, 19, 64, 72, 3, 2),      # stride 2 on odd H and W
    (1, 9, 14, 64, 40, 1, 2),       # the strided 1x1 of a downsample branch
    (2, 6, 10, 160, 136, 1, 1),     # 5 K tiles (K groups 3 + 2 and 2 + 2 + 1 + 0), Cout across 128, Cin no multiple of 64
    (3, 11, 17, 32, 6, 3, 1),       # Cout % 4 != 0
    (2, 8, 8, 64, 64, 3, 1),        # Cout a multiple of every tile width up to 64, M = 128: the in-launch finish
    (1, 42, 50, 32, 136, 1, 1),     # M = 2100: 16 or more tiles and no multiple of 8 for every tile (the XCD run remap)
    # added for the stream-K assertion (more (tile, K tile) units than waves, not a multiple): 66 x 3 tiles of 32 x 64 times 6 K tiles
    # = 1188 units for the 1024 waves of a 256-CU chip.  None of the nine above has more units than a chip has waves.
    (1, 42, 50, 192, 136, 1, 1),
)
VARIANTS = ('none', 'full', 'resmod', 'mask', 'mask_after')
_FLAGS = {      # scale+shift, res, res_mod, mask, mask_after, relu_in, relu_out
    'none':       dict(affine=False, res=False, res_mod=False, mask=False, mask_after=False, relu_in=False, relu_out=False),
    'full':       dict(affine=True, res=True, res_mod=False, mask=False, mask_after=False, relu_in=True, relu_out=True),
    'resmod':     dict(affine=False, res=True, res_mod=True, mask=False, mask_after=False, relu_in=False, relu_out=True),
    'mask':       dict(affine=False, res=True, res_mod=False, mask=True, mask_after=False, relu_in=False, relu_out=False),
    'mask_after': dict(affine=True, res=True, res_mod=False, mask=True, mask_after=True, relu_in=False, relu_out=False),
    # not one of the five VARIANTS: a mask AND both ReLUs, for the NaN launches -- a mask keeps the LDS-tiled kernels off the branch-free
    # buffer epilogue, so this is what reaches the ReLU of the pointer form of the wide epilogue
    'mask_relu':  dict(affine=True, res=True, res_mod=False, mask=True, mask_after=False, relu_in=True, relu_out=True),
}
# gutters of out / res / mask in floats: the 16-byte set takes the wide epilogue when Cout % 4 == 0, the odd set forces the dword one
STRIDES = {'wide': (4, 8, 12), 'odd': (3, 1, 5)}
IN_GUTTER, IN_OFF = 8, 4        # the input: channels [4, 4 + Cin) of rows of Cin + 8 floats


def flags(variant):
    return _FLAGS[variant]


def applies(geom, variant):
    """``resmod`` (a residual shared by the images of the batch) needs two images."""
    return variant != 'resmod' or geom[0] >= 2


def out_hw(geom):
    N, H, W, Cin, Cout, k, s = geom
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def rel(got, ref):
    """max |got - ref| in units of max(|ref|) over ALL elements (NaN where either side has a NaN the other lacks)."""
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def pack(w):
    """[Cout, Cin, kh, kw] -> [Cout, kh * kw * Cin], K ordered (kh, kw, cin) -- what weights.pack_conv_weight gives."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def rb(t):
    return t.bfloat16().to(t.dtype)


def reduced_reference(x, w, stride, pad, mode, double=False):
    """What the reduced-precision kernels compute, in f64: mode 1 = product of the bf16-rounded operands;
    mode 2 (bf16x3) = (xh+xl)*(wh+wl) - xl*wl with x = xh + xl + eps split into two bf16."""
    x, w = x.float(), w.float()
    if mode == 1:
        out = F.conv2d(rb(x).double(), rb(w).double(), stride=stride, padding=pad)
    else:
        xh, wh = rb(x), rb(w)
        xl, wl = rb(x - xh), rb(w - wh)
        full = F.conv2d((xh.double() + xl.double()), (wh.double() + wl.double()), stride=stride, padding=pad)
        out = full - F.conv2d(xl.double(), wl.double(), stride=stride, padding=pad)
    return out if double else out.float()


_reduced_reference = reduced_reference          # the name tests/test_conv_gpu.py imports


def rows(t):
    """NCHW -> [N * H * W, C] (the kernels' row-major NHWC view)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def epilogue(conv, scale, shift, res, res_mod, mask, mask_after, relu_out):
    """The epilogue of vfn_conv_desc on rows [M, Cout], in the dtype of ``conv``:
    act(mask?(conv * scale + shift) + res[row % res_mod]) with the mask before or after the residual."""
    v, dt = conv, conv.dtype
    if scale is not None:
        v = v * scale.to(dt)
    if shift is not None:
        v = v + shift.to(dt)
    if mask is not None and not mask_after:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    if res is not None:
        r = res.to(dt)
        v = v + (r[torch.arange(v.shape[0]) % res_mod] if res_mod else r)
    if mask is not None and mask_after:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    if relu_out:
        v = torch.relu(v)           # (torch.relu keeps a NaN)
    return v


def products(x, w, stride, pad, mode, dtype):
    """The convolution of NCHW ``x`` with ``w`` as rows [M, Cout] in ``dtype`` through F.conv2d: mode 0 exact operands, 1 / 2 the
    products the reduced-precision kernels form (float64: reduced_reference; float32: the same terms summed in float32)."""
    if mode == 0:
        return rows(F.conv2d(x.to(dtype), w.to(dtype), stride=stride, padding=pad))
    if dtype == torch.float64:
        return rows(reduced_reference(x, w, stride, pad, mode, double=True))
    if mode == 1:
        return rows(F.conv2d(rb(x), rb(w), stride=stride, padding=pad))
    xh, wh = rb(x), rb(w)
    xl, wl = rb(x - xh), rb(w - wh)
    c = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)
    return rows(c(xl, wh) + c(xh, wl) + c(xh, wh))


def korder_sum(x, w, stride, mode):
    """Float32 running sum over K in the kernels' order (kh, kw, cin), by unfold: rows [M, Cout]."""
    N, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    cols = F.unfold(x, k, padding=k // 2, stride=stride)                              # [N, Cin * k * k, L], (cin, kh, kw)
    A = cols.view(N, Cin, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * Cin)      # [M, K], (kh, kw, cin)
    B = pack(w)
    terms = [(A, B)]
    if mode == 1:
        terms = [(rb(A), rb(B))]
    elif mode == 2:
        ah, bh = rb(A), rb(B)
        al, bl = rb(A - ah), rb(B - bh)
        terms = [(al, bh), (ah, bl), (ah, bh)]
    acc = torch.zeros(A.shape[0], Cout)
    for kk in range(A.shape[1]):
        for a, b in terms:
            acc += a[:, kk:kk + 1] * b[:, kk]
    return acc


def mask_tensor(M, Cout, g):
    """randn with the values planted that pin ``> 0``: +0, -0, +-FLT_MIN, a whole row <= 0 and a whole row > 0.  No subnormals."""
    m = torch.randn(M, Cout, generator=g)
    flat = m.view(-1)
    plant = (0.0, -0.0, 1.1754944e-38, -1.1754944e-38)
    for i, v in enumerate(plant):
        flat[(i * 7 + 1) % flat.numel()] = v
    if M >= 3:
        m[M // 2] = -m[M // 2].abs()
        m[M // 2, 0] = 0.0
        m[M - 1] = m[M - 1].abs() + 1.1754944e-38
    return m


class Case(dict):
    __getattr__ = dict.__getitem__

    def __hash__(self):
        return id(self)


@functools.lru_cache(maxsize=None)
def make_case(geom, variant, mode=0, nan_at=None):
    """CPU inputs, float64 reference rows [M, Cout], ratio and bound of (geometry, epilogue variant, arithmetic mode); computed once,
    never changed.  ``nan_at`` = (n, h, w, c): that input element is NaN (the bound is the finite case's)."""
    N, H, W, Cin, Cout, k, s = geom
    f = flags(variant)
    g = torch.Generator().manual_seed(1000 + 131 * GEOMS.index(geom) + list(_FLAGS).index(variant))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    Ho, Wo = out_hw(geom)
    M = N * Ho * Wo
    scale = 1 + 0.1 * torch.randn(Cout, generator=g) if f['affine'] else None
    shift = 0.1 * torch.randn(Cout, generator=g) if f['affine'] else None
    res_mod = Ho * Wo if f['res_mod'] else 0
    res = torch.randn(res_mod if res_mod else M, Cout, generator=g) if f['res'] else None
    mask = mask_tensor(M, Cout, g) if f['mask'] else None
    if nan_at is not None:
        finite = make_case(geom, variant, mode)
        x = x.clone()
        x[nan_at[0], nan_at[3], nan_at[1], nan_at[2]] = NAN

    def ep(conv):
        return epilogue(conv, scale, shift, res, res_mod, mask, f['mask_after'], f['relu_out'])
    xin = torch.relu(x) if f['relu_in'] else x
    ref = ep(products(xin, w, s, k // 2, mode, torch.float64))
    if nan_at is None:
        assert bool(torch.isfinite(ref).all())
        ratio = max(rel(ep(products(xin, w, s, k // 2, mode, torch.float32)), ref), rel(ep(korder_sum(xin, w, s, mode)), ref), RATIO_FLOOR)
    else:
        ratio = finite.ratio
    bound = FACTOR * ratio
    if not bound < BOUND_CAP:
        raise ValueError(f'{geom} {variant} mode {mode}: {FACTOR:g} x ratio = {bound:.2e} is not below {BOUND_CAP:g}')
    return Case(geom=geom, variant=variant, mode=mode, flags=f, x=rows(x).contiguous(), w=w, wp=pack(w), scale=scale, shift=shift,
                res=res, res_mod=res_mod, mask=mask, ref=ref, ratio=ratio, bound=bound, M=M, Ho=Ho, Wo=Wo,
                maxref=ref[torch.isfinite(ref)].abs().max().item())


@functools.lru_cache(maxsize=None)
def make_bank_case(banks=3, rows_per_bank=256, cin=64, cout=40, variant='none'):
    """Batched filters (vfn_conv_desc.w_batch_rows): output rows of bank b multiply filter matrix b; a float64 einsum per bank."""
    f = flags(variant)
    g = torch.Generator().manual_seed(77 + VARIANTS.index(variant))
    x = torch.randn(banks, rows_per_bank, cin, generator=g)
    w = torch.randn(banks, cout, cin, generator=g) / cin ** 0.5
    M = banks * rows_per_bank
    scale = 1 + 0.1 * torch.randn(cout, generator=g) if f['affine'] else None
    shift = 0.1 * torch.randn(cout, generator=g) if f['affine'] else None
    res = torch.randn(M, cout, generator=g) if f['res'] else None

    def ep(conv):
        return epilogue(conv, scale, shift, res, 0, None, False, f['relu_out'])
    xin = torch.relu(x) if f['relu_in'] else x
    ref = ep(torch.einsum('brc,boc->bro', xin.double(), w.double()).reshape(M, cout))
    f32 = ep(torch.einsum('brc,boc->bro', xin, w).reshape(M, cout))
    acc = torch.zeros(banks, rows_per_bank, cout)
    for kk in range(cin):
        acc += xin[:, :, kk:kk + 1] * w[:, :, kk].unsqueeze(1)
    ratio = max(rel(f32, ref), rel(ep(acc.reshape(M, cout)), ref), RATIO_FLOOR)
    bound = FACTOR * ratio
    if not bound < BOUND_CAP:
        raise ValueError(f'banks {variant}: {FACTOR:g} x ratio = {bound:.2e} is not below {BOUND_CAP:g}')
    return Case(variant=variant, flags=f, x=x.reshape(M, cin), w=w, scale=scale, shift=shift, res=res, ref=ref, ratio=ratio,
                bound=bound, M=M, banks=banks, rows_per_bank=rows_per_bank, cin=cin, cout=cout, maxref=ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------- layout
def place(data, gutter, off, fill, device):
    """``data`` [R, C] as columns [off, off + C) of rows [GUARD, GUARD + R) of an allocation [R + 2 GUARD, C + gutter] filled with
    ``fill``.  Returns (allocation, view of the data inside it)."""
    R, Cc = data.shape
    assert 0 <= off <= gutter
    alloc = torch.full((R + 2 * GUARD, Cc + gutter), fill, dtype=data.dtype, device=device)
    view = alloc[GUARD:GUARD + R, off:off + Cc]
    view.copy_(data)
    return alloc, view


def bits(t):
    return t.contiguous().view(torch.int32)


class Layout:
    """The tensors of one case laid out for a launch: every one strided and surrounded by poison.

    input   channels [4, 4 + Cin) of rows of Cin + 8 floats
    out     a slice of rows of Cout + STRIDES[set][0] floats, res of Cout + STRIDES[set][1], mask of Cout + STRIDES[set][2]
    poison  gutters and guard rows of input, res and mask: NaN without a ReLU in the launch, +1e30 with one; the output allocation
            holds NaN before every launch (``reset``)."""

    def __init__(self, case, strides, device, x=None):
        fl = case.flags
        self.case, self.strides = case, strides
        self.poison = BIG if (fl['relu_in'] or fl['relu_out']) else NAN
        go, gr, gm = STRIDES[strides]
        cout = case.ref.shape[1]
        self.x_alloc, self.x = place(case.x if x is None else x, IN_GUTTER, IN_OFF, self.poison, device)
        self.in_ld = self.x_alloc.shape[1]
        # (the 16-byte set keeps every slice 16-byte aligned: offsets that are multiples of 4 floats)
        self.out_alloc, self.out = place(torch.full(case.ref.shape, NAN), go, 4 if go % 4 == 0 else 1, NAN, device)
        self.out_ld = cout + go
        self.out_rest = self.out_alloc.clone()
        self.res = self.res_alloc = self.mask = self.mask_alloc = None
        self.res_ld = self.mask_ld = 0
        if case.res is not None:
            self.res_alloc, self.res = place(case.res, gr, 4 if gr % 4 == 0 else 1, self.poison, device)
            self.res_ld = cout + gr
        if case.get('mask') is not None:
            self.mask_alloc, self.mask = place(case.mask, gm, 8 if gm % 4 == 0 else 2, self.poison, device)
            self.mask_ld = cout + gm
        self.scale = case.scale.to(device) if case.scale is not None else None
        self.shift = case.shift.to(device) if case.shift is not None else None
        self.ref = case.ref.to(device)
        self.ref_nan = torch.isnan(self.ref)
        self.ref0 = torch.nan_to_num(self.ref, nan=0.0)

    def collect(self):
        """After a launch: (error in units of max|ref| over every output element -- inf where a NaN is missing or unexpected --,
        1 if any byte of the output allocation outside [:M, :Cout] changed), both on the device; the allocation is at rest again."""
        got = self.out.double()
        got_nan = torch.isnan(got)
        err = (torch.nan_to_num(got, nan=0.0, posinf=1e300, neginf=-1e300) - self.ref0).abs().max() / self.case.maxref
        err = torch.where((got_nan != self.ref_nan).any(), torch.full_like(err, float('inf')), err)
        image = self.out.clone()
        self.out.fill_(NAN)
        dirty = (bits(self.out_alloc) != bits(self.out_rest)).any().double()
        self.out_alloc.copy_(self.out_rest)
        return err, dirty, image


def case_list(mode=0):
    """(geometry, variant) pairs the GPU tests launch in arithmetic mode ``mode``: f32 every geometry x every variant that applies;
    bf16 / bf16x3 the geometries the mode's K tile (64 / 32 channels) divides x the variants 'full' and 'resmod'."""
    kt = 64 if mode == 1 else 32
    variants = VARIANTS if mode == 0 else ('full', 'resmod')
    return [(g, v) for g in GEOMS if g[3] % kt == 0 for v in variants if applies(g, v)]
