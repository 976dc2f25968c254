"""The C-ABI library loads and exports every symbol include/saicv_hip.h declares, and the ctypes binding and the definitions under
csrc/ say what the header says (no compute)."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, 'simpleaicv_pytorch_training_examples_amd', 'libsaicv_hip.so')
HEADER = os.path.join(ROOT, 'include', 'saicv_hip.h')


def _declared():
    return sorted(set(re.findall(r'\b(saicv_[a-z0-9_]+)\s*\(', open(HEADER).read())))


def test_header_declares_entry_points():
    names = _declared()
    assert len(names) >= 25
    for must in ('saicv_conv2d_fwd', 'saicv_conv2d_dgrad', 'saicv_conv2d_wgrad', 'saicv_bn_act_fwd',
                 'saicv_bn_act_bwd', 'saicv_softmax_ce_fwd', 'saicv_sgd_flat', 'saicv_last_error_string'):
        assert must in names


@pytest.mark.skipif(not os.path.exists(LIB), reason='library not built (run __graft_entry__.build())')
def test_library_exports_every_declared_symbol():
    handle = ctypes.CDLL(LIB)
    missing = [n for n in _declared() if not hasattr(handle, n)]
    assert not missing, missing
    handle.saicv_version.restype = ctypes.c_int
    assert handle.saicv_version() >= 100


@pytest.mark.skipif(not os.path.exists(LIB), reason='library not built')
def test_python_binding_covers_header():
    from simpleaicv_pytorch_training_examples_amd import _lib
    declared = set(_declared())
    bound = set(_lib.SIGNATURES)
    assert declared == bound, sorted(declared ^ bound)
    # error path works without a GPU: a null descriptor is rejected, message is readable
    L = _lib.lib()
    assert L.saicv_conv2d_stat_rows(None) == -1
    rc = L.saicv_conv2d_fwd(None, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rc != 0 and b'null descriptor' in L.saicv_last_error_string()


STRUCTS = {'saicv_conv_desc': 'ConvDesc', 'saicv_attn_desc': 'AttnDesc', 'saicv_dgrad_fuse': 'DgradFuse', 'saicv_plan_query': 'PlanQuery',
           'saicv_plan': 'Plan', 'saicv_pack_desc': 'PackDesc', 'saicv_mix_plan': 'MixPlan', 'saicv_erase_box': 'EraseBox'}


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof of the header's eight structs, as a C compiler lays them out, against the ctypes classes."""
    from simpleaicv_pytorch_training_examples_amd import _lib
    cc = next((c for c in ('/opt/rocm/llvm/bin/clang', shutil.which('cc')) if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip('no host C compiler')
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    want = {}
    for cname, pyname in STRUCTS.items():
        cls = getattr(_lib, pyname)
        assert issubclass(cls, ctypes.Structure) and len(cls._fields_) >= 7, pyname
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        want[cname] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            lines.append(f'    printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
            want[f'{cname}.{field}'] = getattr(cls, field).offset
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.check_call([cc, '-std=c99', '-o', str(exe), str(src)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got == want
    # the field lists themselves are the header's: a member the parser dropped would still leave equal offsets for the rest
    header = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for cname, pyname in STRUCTS.items():
        body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', header, flags=re.S).group(1)
        members = [re.search(r'(\w+)(?:\[\d+\])?\s*$', d).group(1) for stmt in body.split(';') if stmt.strip() for d in stmt.split(',')]
        assert members == [f for f, _ in getattr(_lib, pyname)._fields_], cname
    assert _lib.EraseBox.color.size == 16 and _lib.PlanQuery.conv.size == ctypes.sizeof(_lib.ConvDesc)


def test_binding_signatures_written_out_by_hand():
    """A representative few argtypes lists, typed here from the header by hand: the parser is not its own reference."""
    from simpleaicv_pytorch_training_examples_amd import _lib
    P = c_void_p
    assert _lib.SIGNATURES['saicv_bn_act_fwd_stats'] == (c_int, [
        c_int, P, P, P, P, P, c_int, c_double, P, P, P, P, c_double, c_double, P, P, P, c_size_t, c_int, c_int, P, P])
    assert _lib.SIGNATURES['saicv_ctc_loss_bwd'] == (c_int, [
        c_int, P, c_longlong, c_longlong, P, c_longlong, c_longlong, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_float, P])
    assert _lib.SIGNATURES['saicv_trimap_stats_fwd'] == (c_int, [
        P, ctypes.c_long, ctypes.c_long, ctypes.c_long, P, c_int, c_size_t, c_float, P, P, P])
    assert _lib.SIGNATURES['saicv_last_error_string'] == (c_char_p, [])
    assert _lib.SIGNATURES['saicv_c3_bwd_stream_ws_floats'] == (c_size_t, [c_int, c_int, c_int])
    res, args = _lib.SIGNATURES['saicv_attention_stream_fwd']
    assert res is c_int and args == [c_int, c_int, _lib.struct_ptr(_lib.AttnDesc), P]
    # a struct pointer takes byref() of its own struct, None or an address, and nothing else
    desc = args[2]
    assert desc.struct is _lib.AttnDesc
    desc.from_param(ctypes.byref(_lib.AttnDesc()))
    assert desc.from_param(None).value is None and desc.from_param(4096).value == 4096
    with pytest.raises(TypeError):
        desc.from_param(ctypes.byref(_lib.ConvDesc()))
    # out-parameters of the communicator calls are passed with byref()
    for argtype, value in zip(_lib.SIGNATURES['saicv_comm_stats'][1],
                              [c_void_p(), ctypes.byref(c_int()), ctypes.byref(c_int()), ctypes.byref(ctypes.c_ulonglong()),
                               ctypes.byref(ctypes.c_ulonglong())]):
        argtype.from_param(value)
    assert _lib.SIGNATURES['saicv_comm_create'][1][3].from_param(ctypes.byref(c_void_p())) is not None
    assert (_lib.BF16, _lib.F32, _lib.PLAN_CONV_FWD, _lib.PLAN_LINEAR_WGRAD, _lib.ROUTE_TILED, _lib.ROUTE_TN) == (0, 1, 0, 5, 0, 3)


def test_header_parser_is_strict():
    from simpleaicv_pytorch_training_examples_amd import _lib
    good = '#define SAICV_X 3\ntypedef struct saicv_t { int a, b; float c[2]; const void* p; } saicv_t;\n' \
           'int saicv_f(const saicv_t* t, long long n, void* stream);\nsize_t saicv_g(void);\n'
    constants, structs, signatures = _lib.parse_header(good)
    assert constants == {'SAICV_X': 3}
    T = structs['saicv_t']
    assert [f for f, _ in T._fields_] == ['a', 'b', 'c', 'p'] and (T.c.offset, T.p.offset, ctypes.sizeof(T)) == (8, 16, 24)
    assert signatures == {'saicv_f': (c_int, [_lib.struct_ptr(T), c_longlong, c_void_p]), 'saicv_g': (c_size_t, [])}
    for bad in ('int saicv_f(int a, short b);',                         # a type the binding does not know
                'int saicv_f(saicv_unknown* p);',
                'typedef struct saicv_t { int a; wchar_t b; } saicv_t;',
                'int saicv_f(int a, int (*callback)(int));',            # declarations it cannot split
                'int saicv_f(int a, long long);',
                'int saicv_f(int a[4]);',
                'typedef struct saicv_t { float* a, b; } saicv_t;',
                'int saicv_f(int a)',
                'int saicv_f(int a); int saicv_f(int a);',
                'int other_f(int a);'):
        with pytest.raises(ValueError):
            _lib.parse_header(good + bad)


def test_every_entry_point_is_defined_once_under_its_declaration():
    """A definition with the header in scope cannot drift from it (the compiler refuses conflicting types), so: every unit that
    defines an entry point includes the header, and every declared name has exactly one definition."""
    definition = re.compile(r'^(?:extern "C" )?(?:int|size_t|const char\*) (saicv_\w+)\([^;{]*\)\s*\{', flags=re.M)
    defined = []
    for path in sorted(glob.glob(os.path.join(ROOT, 'simpleaicv_pytorch_training_examples_amd', 'csrc', '*.hip'))):
        text = open(path).read()
        names = definition.findall(text)
        if names:
            assert re.search(r'^#include ".*include/saicv_hip\.h"', text, flags=re.M), os.path.basename(path)
        defined += names
    assert sorted(defined) == _declared()


def test_integration_guide_names_every_entry_point():
    """INTEGRATION.md maps each exported symbol to the reference call it replaces: none may be missing from that table
    (families are written as `saicv_x_fwd / _bwd`: a documented stem plus a documented suffix)."""
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    missing = []
    for name in _declared():
        if name in doc:
            continue
        cuts = [i for i, ch in enumerate(name) if ch == '_' and i > len('saicv')]
        if any(('`' + name[:i]) in doc and re.search(r'[ /`]' + re.escape(name[i:]) + r'\b', doc) for i in cuts):
            continue
        if any(('`' + name[:i] + '_*`') in doc for i in cuts):          # `saicv_maxpool_*`
            continue
        missing.append(name)
    assert not missing, missing
