"""ctypes binding of ``libvfn_hip.so``, derived from the one declaration of its C ABI, ``include/vfn_hip.h``.

The library is the product: if it is missing, or a launcher reports a non-zero
status, this module raises ``RuntimeError`` -- there is no eager / CPU fallback.
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VFN_LIB_PATH') or os.path.join(_HERE, 'libvfn_hip.so')     # (override: ablation builds, scripts/)

_lib = None

c_fp = C.c_void_p          # device pointers travel as void*

# ---------------------------------------------------------------------------------------------- the header, read as text
# One rule for every field and parameter: a scalar is the matching ctypes scalar, ``T name[N]`` in a struct is ``ctype * N``,
# ``char*`` is c_char_p, a parameter that points at a struct of the header is POINTER(that struct) -- unless its name ends in
# ``_dev``, the header's convention for a table that lives in device memory -- and every other pointer is c_void_p.
_SCALARS = {'int': C.c_int, 'float': C.c_float, 'double': C.c_double, 'long long': C.c_longlong}
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned char', 'short', 'unsigned short', 'unsigned long long'}     # what a pointer may name
_RENAMED = {'in': 'inp'}   # field names that are Python keywords
_DECLARATOR = re.compile(r'(?:const\s+)?([A-Za-z_][\w ]*?)(?:\s*(\*)\s*|\s+)(\w+)\s*(?:\[([^\]]*)\])?')


def parse_header(text, known_structs=None):
    """``(defines, enums, structs, prototypes)`` of a header in the style of ``include/vfn_hip.h``: the integer ``#define``s
    and ``enum`` values by name, a ``ctypes.Structure`` per ``typedef struct`` and the ``argtypes`` of every ``int vfn_*(...)``.
    Anything else -- an unknown base type, an array bound that does not evaluate, an unbalanced declaration -- is a
    ``RuntimeError`` that names the declaration; nothing is skipped.  ``known_structs``: the structs of a header this one builds on
    (a later part of the ABI that takes descriptors of ``vfn_hip.h``); they are not returned again."""
    defines, enums, structs, protos = {}, {}, dict(known_structs or {}), {}

    def fail(why, decl):
        raise RuntimeError(f'vfn_hip.h: {why}: {" ".join(decl.split())[:120]!r}')

    def number(expr, decl):
        try:
            if not re.fullmatch(r'[\w\s()+*-]+', expr):
                raise ValueError(expr)
            return int(eval(expr, {'__builtins__': {}}, {**defines, **enums}))
        except Exception:
            fail(f'cannot evaluate {expr.strip()!r}', decl)

    def declarator(item, decl, param):
        m = _DECLARATOR.fullmatch(item.strip())
        if not m:
            fail('declaration not understood', decl)
        base, star, name, bound = ' '.join(m.group(1).split()), m.group(2), m.group(3), m.group(4)
        if base not in _POINTEES and base not in structs:
            fail(f'unknown base type {base!r}', decl)
        if bound is not None and (star or param):
            fail('array of pointers or array parameter', decl)
        if star:
            if base == 'char':
                t = C.c_char_p
            elif base in structs and param and not name.endswith('_dev'):
                t = C.POINTER(structs[base])
            else:
                t = C.c_void_p
        elif base in _SCALARS:
            t = _SCALARS[base]
        elif base in structs and not param:
            t = structs[base]
        else:
            fail(f'{base!r} by value', decl)
        return _RENAMED.get(name, name), t if bound is None else t * number(bound, decl)

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$', ' ', text, flags=re.S | re.M)     # extern "C" { / }
    code = []
    for line in text.split('\n'):
        if not line.lstrip().startswith('#'):
            code.append(line)
        elif not re.fullmatch(r'\s*#\s*(ifndef\s+\w+|define\s+\w+|endif)\s*', line):     # (those: the include guard)
            m = re.fullmatch(r'\s*#\s*define\s+(\w+)\b(?!\()(.+)', line)
            if not m:
                fail('directive not understood', line)
            defines[m.group(1)] = number(m.group(2), line)
    text = '\n'.join(code)

    decls, depth, start = [], 0, 0
    for pos, ch in enumerate(text):
        depth += (ch == '{') - (ch == '}')
        if depth < 0:
            fail('unbalanced declaration', text[start:pos + 1])
        if ch == ';' and depth == 0:
            decls.append(text[start:pos])
            start = pos + 1
    if text[start:].strip():
        fail('unbalanced declaration', text[start:])

    for decl in decls:
        m = re.fullmatch(r'\s*enum\s*\{(.*)\}\s*', decl, flags=re.S)
        if m:
            value = -1
            for item in m.group(1).split(','):
                name, _, expr = item.partition('=')
                value = number(expr, decl) if expr.strip() else value + 1
                enums[name.strip()] = value
            continue
        m = re.fullmatch(r'\s*typedef\s+struct\s*(\w*)\s*\{(.*)\}\s*(\w+)\s*', decl, flags=re.S)
        if m:
            if m.group(1) not in ('', m.group(3)):
                fail('struct tag and typedef name differ', decl)
            fields = []
            for member in m.group(2).split(';'):
                if member.strip():
                    first, *more = member.split(',')
                    head = _DECLARATOR.fullmatch(first.strip())
                    if more and (not head or head.group(2)):
                        fail('several declarators after a pointer', member)
                    fields.append(declarator(first, member, False))
                    fields += [declarator(f'{head.group(1)} {item}', member, False) for item in more]
            structs[m.group(3)] = type(m.group(3), (C.Structure,), {'_fields_': fields})
            continue
        m = re.fullmatch(r'\s*int\s+(vfn_\w+)\s*\((.*)\)\s*', decl, flags=re.S)
        if m:
            if m.group(1) in protos:
                fail('declared twice', decl)
            params = m.group(2).strip()
            protos[m.group(1)] = [] if params == 'void' else [declarator(p, decl, True)[1] for p in params.split(',')]
            continue
        fail('declaration not understood', decl)
    return defines, enums, {k: v for k, v in structs.items() if k not in (known_structs or {})}, protos


with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_hip.h')) as _f:
    DEFINES, ENUMS, STRUCTS, SIGNATURES = parse_header(_f.read())     # SIGNATURES: name -> argtypes (restype is int everywhere)
ALL_SYMBOLS = sorted(SIGNATURES)
# the second part of the ABI (entry points only, no structs): Winograd F(6x6, 3x3), include/vfn_winograd6.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_winograd6.h')) as _f:
    SIGNATURES_WINOGRAD6 = parse_header(_f.read())[3]
# the third part (entry points only, no structs): samples and scores of the image model's validation, include/vfn_image_val.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_image_val.h')) as _f:
    DEFINES_IMAGE_VAL, _, _, SIGNATURES_IMAGE_VAL = parse_header(_f.read())
# the fourth part (entry points only, on the descriptors of vfn_hip.h): a block's shortcut convolution inside conv3's launch,
# include/vfn_shortcut_fused.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_shortcut_fused.h')) as _f:
    SIGNATURES_SHORTCUT_FUSED = parse_header(_f.read(), STRUCTS)[3]
# the fifth part (one entry point on vfn_conv_desc): the LDS-resident 3x3 convolution of the 32-filter layers, include/vfn_conv_thin.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_conv_thin.h')) as _f:
    DEFINES_CONV_THIN, _, _, SIGNATURES_CONV_THIN = parse_header(_f.read(), STRUCTS)
# the sixth part (entry points only, no structs): fine-tuning the LinkNet decoder and head, include/vfn_image_train.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_image_train.h')) as _f:
    DEFINES_IMAGE_TRAIN, _, _, SIGNATURES_IMAGE_TRAIN = parse_header(_f.read())
LNT_MAX_BLOCKS, LNT_MAX_C = DEFINES_IMAGE_TRAIN['VFN_LNT_MAX_BLOCKS'], DEFINES_IMAGE_TRAIN['VFN_LNT_MAX_C']
# the seventh part (entry points only, no structs): the encoder's backward with frozen statistics, include/vfn_encoder_train.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_encoder_train.h')) as _f:
    DEFINES_ENCODER_TRAIN, _, _, SIGNATURES_ENCODER_TRAIN = parse_header(_f.read())
ET_MAX_BLOCKS, ET_MAX_SQ = DEFINES_ENCODER_TRAIN['VFN_ET_MAX_BLOCKS'], DEFINES_ENCODER_TRAIN['VFN_ET_MAX_SQ']
# the eighth part (entry points only, no structs): the encoder in train mode, batch-statistics BatchNorm and drop-connect,
# include/vfn_encoder_bn_train.h
with open(os.path.join(os.path.dirname(_HERE), 'include', 'vfn_encoder_bn_train.h')) as _f:
    SIGNATURES_ENCODER_BN_TRAIN = parse_header(_f.read())[3]
SEG_SCORES_CHUNK, SEG_SCORES_MAX_BLOCKS = DEFINES_IMAGE_VAL['VFN_SEG_SCORES_CHUNK'], DEFINES_IMAGE_VAL['VFN_SEG_SCORES_MAX_BLOCKS']
ABI_VERSION = DEFINES['VFN_ABI_VERSION']
TRAIN_AUG_MAX_T, TRAIN_AUG_MAX_SIDE, TRAIN_AUG_MAX_OUT, TRAIN_AUG_MAX_OBJ = (
    DEFINES['VFN_TRAIN_AUG_MAX_' + _k] for _k in ('T', 'SIDE', 'OUT', 'OBJ'))

ConvDesc = STRUCTS['vfn_conv_desc']
WgradDesc = STRUCTS['vfn_wgrad_desc']
RefreshFilter = STRUCTS['vfn_refresh_filter']
RefreshEpilogue = STRUCTS['vfn_refresh_epilogue']
GatherEntry = STRUCTS['vfn_gather_entry']
StemDesc = STRUCTS['vfn_stem_desc']
BankScanDesc = STRUCTS['vfn_bankscan_desc']
MemReadDesc = STRUCTS['vfn_memread_desc']
BankMatchDesc = STRUCTS['vfn_bankmatch_desc']
BankDesc = STRUCTS['vfn_bank_desc']
TrainAugFrame = STRUCTS['vfn_train_aug_frame']
TrainAugDesc = STRUCTS['vfn_train_aug_desc']

# vfn_sizeof_desc(which): the pairing of csrc/abi.hip's switch
DESC_IDS = {ENUMS['VFN_DESC_' + _k]: _c for _k, _c in (
    ('CONV', ConvDesc), ('STEM', StemDesc), ('BANKSCAN', BankScanDesc), ('MEMREAD', MemReadDesc), ('BANK', BankDesc),
    ('WGRAD', WgradDesc), ('REFRESH_FILTER', RefreshFilter), ('REFRESH_EPILOGUE', RefreshEpilogue), ('GATHER', GatherEntry),
    ('BANKMATCH', BankMatchDesc), ('TRAIN_AUG', TrainAugDesc))}


def lib():
    """Load the shared library once; raise loudly if it is absent or stale."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build the HIP kernels first '
                '(python -c "import __graft_entry__ as g; g.build()" or make -C v-floodnet_amd/csrc)')
        L = C.CDLL(LIB_PATH)

        def declare(name, signatures=SIGNATURES, header='vfn_hip.h'):
            if not hasattr(L, name):
                raise RuntimeError(f'{LIB_PATH} lacks {name}, which include/{header} declares: rebuild it (make -C v-floodnet_amd/csrc)')
            fn = getattr(L, name)
            fn.argtypes, fn.restype = signatures[name], C.c_int
            return fn

        if declare('vfn_abi_version')() != ABI_VERSION:
            raise RuntimeError(f'{LIB_PATH} has ABI version {L.vfn_abi_version()}, this package expects {ABI_VERSION} '
                               '(descriptor layouts differ): rebuild it (make -C v-floodnet_amd/csrc)')
        declare('vfn_sizeof_desc')
        for which, cls in DESC_IDS.items():
            if L.vfn_sizeof_desc(which) != C.sizeof(cls):
                raise RuntimeError(f'{LIB_PATH}: sizeof({cls.__name__}) is {L.vfn_sizeof_desc(which)} in the library, '
                                   f'{C.sizeof(cls)} in this binding: rebuild it (make -C v-floodnet_amd/csrc)')
        for name in SIGNATURES:
            declare(name)
        for name in SIGNATURES_WINOGRAD6:
            declare(name, SIGNATURES_WINOGRAD6, 'vfn_winograd6.h')
        for name in SIGNATURES_IMAGE_VAL:
            declare(name, SIGNATURES_IMAGE_VAL, 'vfn_image_val.h')
        for name in SIGNATURES_SHORTCUT_FUSED:
            declare(name, SIGNATURES_SHORTCUT_FUSED, 'vfn_shortcut_fused.h')
        for name in SIGNATURES_CONV_THIN:
            declare(name, SIGNATURES_CONV_THIN, 'vfn_conv_thin.h')
        for name in SIGNATURES_IMAGE_TRAIN:
            declare(name, SIGNATURES_IMAGE_TRAIN, 'vfn_image_train.h')
        for name in SIGNATURES_ENCODER_TRAIN:
            declare(name, SIGNATURES_ENCODER_TRAIN, 'vfn_encoder_train.h')
        for name in SIGNATURES_ENCODER_BN_TRAIN:
            declare(name, SIGNATURES_ENCODER_BN_TRAIN, 'vfn_encoder_bn_train.h')
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f'HIP kernel launcher {what} failed with status {status}')


def ptr(t):
    """Device pointer of a tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream():
    """hipStream_t of torch's current stream on the current device (one C call: this runs before every kernel launch)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(t, what='tensor'):
    if not t.is_cuda:
        raise RuntimeError(f'{what} must live on the GPU: the V-FloodNet hot path has no CPU fallback')


# ---------------------------------------------------------------------------------------------- streams that really run beside each other
# A HIP stream is not a hardware queue.  The runtime multiplexes every stream of a priority onto a few hardware queues
# (GPU_MAX_HW_QUEUES, default 4), and PyTorch creates its whole pool of 32 streams per priority on the first
# ``torch.cuda.Stream()``: streams that share a hardware queue execute IN ORDER, whatever their events say.  Round 6 found the
# PNG sink's stream on the queue of the frame loop's stream: its five latency-bound kernels per image ran between two frames
# instead of underneath the next one -- 0.85 ms of an idle matrix pipe per frame in ``video_seg.main`` (median gap between a
# frame's last marker and the next frame's first: 0.855 ms; 0.012 ms with 24 hardware queues, which is no cure: the command
# processor then time-slices and the loop runs at 76 frames/s).  So side streams are PICKED: a candidate is kept only if a tiny
# kernel on it finishes while every stream in ``beside`` is still busy with a few milliseconds of queued work.
PROBES = []          # (found, candidates tried) of every independent_stream call of this process (bench.py reports them)


def independent_stream(device, beside=(), tries=12, priority=0):
    """A ``torch.cuda.Stream`` whose hardware queue is not the one of the current stream nor of any stream in ``beside``
    (measured, see above).  Falls back to the last candidate if none qualifies within ``tries`` (the loop then still works,
    serialised as before)."""
    device = torch.device(device)
    cur = torch.cuda.current_stream(device)
    others = [cur] + [s_ for s_ in beside if s_ is not None]
    big, small = torch.zeros(16 * 1024 * 1024, device=device), torch.zeros(16, device=device)     # (64 MB, returned to the allocator at exit)

    def overlaps(cand, ref):
        torch.cuda.synchronize(device)
        ref_end, cand_end = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(ref):
            for _ in range(64):                     # ~2 ms of bandwidth-bound work queued on ``ref``
                big.add_(1.0)
            ref_end.record()
        with torch.cuda.stream(cand):
            small.add_(1.0)
            cand_end.record()
        cand_end.synchronize()
        ok = not ref_end.query()                    # the candidate's kernel finished while ``ref`` was still busy
        torch.cuda.synchronize(device)
        return ok

    cand = None
    for n_ in range(tries):
        cand = torch.cuda.Stream(device=device, priority=priority)
        if all(overlaps(cand, o_) for o_ in others):
            PROBES.append((True, n_ + 1))
            return cand
    PROBES.append((False, tries))
    import warnings
    warnings.warn('vfloodnet_amd: no stream with a hardware queue of its own found; side-stream work will run in order with the frame loop')
    return cand
