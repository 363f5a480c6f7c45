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
