"""The C-ABI library loads and exports every symbol include/vfn_hip.h declares (no GPU needed)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'vfn_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\bint\s+(vfn_\w+)\s*\(', txt)))


def test_header_and_binding_agree():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    assert declared_symbols() == _lib.ALL_SYMBOLS


def test_library_exports_every_declared_symbol():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    for s in declared_symbols():
        assert hasattr(L, s), s
    hdr = open(os.path.join(ROOT, 'include', 'vfn_hip.h')).read()
    assert L.vfn_abi_version() == _lib.ABI_VERSION == int(re.search(r'#define VFN_ABI_VERSION (\d+)', hdr).group(1))
    assert L.vfn_conv_cfg_count() == 62


def test_conv_cfg_table_is_the_recorded_one():
    """The configuration ids are persisted in tuned_gfx950*.json, so what an id means is a file format.  tests/golden/conv_cfgs.json
    is what the queries answered for all 62 ids before the table in csrc/conv_igemm.hip drove queries and launches (dumped from
    the library of that commit: vfn_conv_cfg_info / _wk / _tpb / _kind and ops.conv_cfg_names for the three modes); the library
    must reproduce it exactly.  vfn_conv_cfg_modes must give all three modes to the ids the reduced-precision entry points
    accepted then, f32 alone to every other id, and nothing out of range."""
    import ctypes as C
    import json
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib, ops
    L = _lib.lib()
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_cfgs.json')))
    assert [r['id'] for r in golden] == list(range(62)) and L.vfn_conv_cfg_count() == 62
    names = [ops.conv_cfg_names(m) for m in (0, 1, 2)]
    for r in golden:
        c = r['id']
        v = [C.c_int(-7) for _ in range(5)]
        assert L.vfn_conv_cfg_info(c, *[C.byref(x) for x in v]) == 0
        got = {'id': c, 'info': [x.value for x in v], 'wk': L.vfn_conv_cfg_wk(c), 'tpb': L.vfn_conv_cfg_tpb(c),
               'kind': L.vfn_conv_cfg_kind(c), 'names': [names[m][c] for m in range(3)]}
        assert got == r
    all_modes = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 17, 19, 22, 23) + tuple(range(26, 38))
    for c in range(62):
        assert L.vfn_conv_cfg_modes(c) == (7 if c in all_modes else 1), c
    assert ops.conv_cfgs(0) == tuple(range(62)) and ops.conv_cfgs(1) == ops.conv_cfgs(2) == all_modes
    assert ops.BF16_CFGS == all_modes                                                         # (the earlier name, now asked of the library)
    buf = C.create_string_buffer(96)
    for c in (-1, 62):
        assert L.vfn_conv_cfg_modes(c) == 0 and L.vfn_conv_cfg_wk(c) == 0 and L.vfn_conv_cfg_tpb(c) == 0 and L.vfn_conv_cfg_kind(c) == -1
        assert L.vfn_conv_cfg_info(c, *[C.byref(C.c_int()) for _ in range(5)]) == 1           # VFN_ERR_ARG
        assert L.vfn_conv_cfg_name(c, buf, 96) == 1
    for c in range(38):
        assert L.vfn_conv_cfg_name(c, buf, 96) == 1                                            # kind 0: names come from _info


def test_descriptor_sizes_match_the_library():
    """A binding whose ctypes struct drifted from include/vfn_hip.h is caught here (and at load time)."""
    import ctypes as C
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    L = _lib.lib()
    for which, cls in _lib.DESC_IDS.items():
        assert L.vfn_sizeof_desc(which) == C.sizeof(cls), cls.__name__
    assert L.vfn_sizeof_desc(99) == -1
    names = __import__('vfloodnet_amd').ops.conv_cfg_names(0)
    assert names[10] == 'conv_igemm_kernel<64, 128, 2, 4, 0>' and names[13] == 'conv_igemm_dma_kernel<64, 64, 2, 2, 2>'


def test_missing_library_fails_loudly(monkeypatch):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libvfn_hip.so')
    with pytest.raises(RuntimeError):
        _lib.lib()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'v-floodnet_amd')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert 'import oracle' not in src and 'from oracle' not in src, fn


# ---------------------------------------------------------------------------------------------- the binding is derived from the header
def _hipcc():
    """The compiler of v-floodnet_amd/csrc/Makefile (HIPCC ?= hipcc)."""
    import shutil
    return shutil.which(os.environ.get('HIPCC', 'hipcc')) or shutil.which('/opt/rocm/bin/hipcc')


def _c_type(t):
    """The C spelling of a derived field type, or None for a pointer (every pointer field travels as void*)."""
    import ctypes as C
    from vfloodnet_amd import _lib
    if hasattr(t, '_length_'):
        return f'{_c_type(t._type_)}[{t._length_}]'
    names = {C.c_int: 'int', C.c_float: 'float', C.c_double: 'double', C.c_longlong: 'long long', C.c_void_p: None}
    return names[t] if t in names else {c: n for n, c in _lib.STRUCTS.items()}[t]


def test_compiler_agrees_with_the_derived_structs(tmp_path):
    """One translation unit of static_asserts -- sizeof of every struct; offset, size and C type of every field as the parser derived
    them -- compiled host-only (syntax check: no device code, nothing runs) against include/vfn_hip.h."""
    import ctypes as C
    import subprocess
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    cc = _hipcc()
    if cc is None:
        pytest.skip('no hipcc on this machine')
    c_name = {py: c for c, py in _lib._RENAMED.items()}
    lines = ['#include <cstddef>', '#include <type_traits>', '#include "vfn_hip.h"']
    assert len(_lib.STRUCTS) == 12
    for sname, cls in _lib.STRUCTS.items():
        lines.append(f'static_assert(sizeof({sname}) == {C.sizeof(cls)}, "sizeof {sname}");')
        for fname, ftype in cls._fields_:
            f, d, ct = c_name.get(fname, fname), getattr(cls, fname), _c_type(ftype)
            lines.append(f'static_assert(offsetof({sname}, {f}) == {d.offset} && sizeof((({sname}*)0)->{f}) == {d.size}, "{sname}.{f}");')
            kind = f'std::is_same<decltype({sname}::{f}), {ct}>' if ct else f'std::is_pointer<decltype({sname}::{f})>'
            lines.append(f'static_assert({kind}::value, "type of {sname}.{f}");')
    src = tmp_path / 'abi_layout.cpp'
    src.write_text('\n'.join(lines) + '\n')
    r = subprocess.run([cc, '-x', 'c++', '-std=c++11', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_prototypes_are_derived_by_the_type_rule():
    import ctypes as C
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    S = _lib.SIGNATURES
    i, p, ll, d = C.c_int, C.c_void_p, C.c_longlong, C.c_double
    assert sorted(S) == declared_symbols() and len(S) == 111
    assert S['vfn_abi_version'] == []
    assert S['vfn_conv_cfg_name'] == [i, C.c_char_p, i]
    assert S['vfn_conv2d_nhwc_f32'] == [C.POINTER(_lib.ConvDesc), i, p]
    assert S['vfn_conv1x1_persistent_f32'] == [C.POINTER(_lib.ConvDesc), i, i, p]
    assert S['vfn_refresh_filters_f32'] == [p, i, i, p]                                      # table_dev: a struct pointer named *_dev
    assert S['vfn_refresh_epilogues_f32'][0] is p and S['vfn_gather_strided_f32'][0] is p
    assert S['vfn_adamw_f32'] == [p, p, p, p, ll, d, d, d, d, d, i, p]
    assert S['vfn_winograd_output_f32'] == [p, i, i, i, i, i, p, p, p, i, i, i, p, i, p]     # a prototype that spans lines
    assert S['vfn_scatter_mean_checked_f32'] == [p, ll, ll, p, ll, i, p, ll, ll, i, ll, p, p]   # const long long* -> void*
    assert S['vfn_jpeg_idct_u8'] == [p, p, p, i, i, i, p]                                    # short*, unsigned short* -> void*
    assert S['vfn_softmax_cols_f32'] == [p, i, i, i, C.c_float, p, p]
    assert S['vfn_bank_refresh_norms'] == [C.POINTER(_lib.BankDesc), p, p, p, p]
    assert C.POINTER(_lib.ConvDesc) is C.POINTER(_lib.STRUCTS['vfn_conv_desc']) and _lib.ConvDesc._fields_[0][0] == 'inp'
    assert _lib.TrainAugDesc.frame.size == 16 * C.sizeof(_lib.TrainAugFrame) and _lib.TrainAugDesc.obj_list.size == 40


def test_parser_refuses_what_it_does_not_understand():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd._lib import parse_header
    ok = 'typedef struct vfn_s { const float* in; int n[VFN_N - 1]; } vfn_s;\nint vfn_f(const vfn_s* d, const vfn_s* t_dev, void* stream);\n'
    defines, enums, structs, protos = parse_header('#define VFN_N (2 * 2)\nenum { VFN_A = 3, VFN_B };\n' + ok)
    assert defines == {'VFN_N': 4} and enums == {'VFN_A': 3, 'VFN_B': 4} and [f[0] for f in structs['vfn_s']._fields_] == ['inp', 'n']
    assert structs['vfn_s'].n.size == 12 and protos['vfn_f'][1:] == [__import__('ctypes').c_void_p] * 2
    for bad, names in (('typedef struct { size_t n; } vfn_s;', 'size_t'),                    # an unknown base type
                       ('typedef struct { int n[VFN_NOT_DEFINED]; } vfn_s;', 'VFN_NOT_DEFINED'),   # a bound that does not evaluate
                       ('#define VFN_N 4\n' + ok + 'int vfn_g(vfn_s d);', 'vfn_g'),            # a struct by value
                       ('#define VFN_N 4\n' + ok + 'int vfn_g(size_t n);', 'vfn_g'),
                       ('#define VFN_N 4\n' + ok + 'int vfn_g(int n)', 'vfn_g'),               # unbalanced: no terminator
                       ('typedef struct { int n; vfn_s;', 'int n'),
                       ('int vfn_g(int n);\n}', 'unbalanced'),
                       ('float vfn_g(int n);', 'vfn_g'),                                       # every entry point returns int
                       ('int vfn_g(int n);\nint vfn_g(int n);', 'vfn_g'),
                       ('#define VFN_F(x) 1', 'VFN_F'), ('#include <stddef.h>', 'stddef')):
        with pytest.raises(RuntimeError, match=names):
            parse_header(bad)


def test_constants_come_from_the_header():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib, ops, feature_bank, backward
    hdr = open(os.path.join(ROOT, 'include', 'vfn_hip.h')).read()

    def define(name):
        return eval(re.search(r'#define ' + name + r' ([\d\s()*]+)', hdr).group(1))

    assert _lib.ABI_VERSION == define('VFN_ABI_VERSION') == 18
    assert ops.SK_WS_FLOATS == define('VFN_CONV_SK_WS_FLOATS') == 16 * 1024 * 1024
    assert ops.SK_MAX_TILES == define('VFN_CONV_SK_MAX_TILES') == 16384
    assert feature_bank.MAX_HW == define('VFN_BANK_MAX_HW') == 32768
    assert (_lib.TRAIN_AUG_MAX_T, _lib.TRAIN_AUG_MAX_SIDE, _lib.TRAIN_AUG_MAX_OUT, _lib.TRAIN_AUG_MAX_OBJ) == tuple(
        define('VFN_TRAIN_AUG_MAX_' + k) for k in ('T', 'SIDE', 'OUT', 'OBJ')) == (16, 8192, 4096, 11)
    assert backward.COLSUM_COUNTERS == define('VFN_COLSUM_COUNTERS') == 64
    src = open(os.path.join(ROOT, 'v-floodnet_amd', 'backward.py')).read()                    # every ticket buffer has that length
    assert len(re.findall(r'self\._ticket\w* = torch\.zeros\(COLSUM_COUNTERS, dtype=torch\.int32', src)) == len(re.findall(r'self\._ticket\w* = ', src)) == 6
    assert {_lib.DESC_IDS[_lib.ENUMS[k]].__name__ for k in _lib.ENUMS} == set(_lib.STRUCTS) - {'vfn_train_aug_frame'}


def test_a_declared_symbol_the_library_lacks_is_named(monkeypatch):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setitem(_lib.SIGNATURES, 'vfn_not_in_the_library', [])
    with pytest.raises(RuntimeError, match='vfn_not_in_the_library'):
        _lib.lib()
