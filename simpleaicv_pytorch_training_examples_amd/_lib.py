"""ctypes binding of libsaicv_hip.so, read from include/saicv_hip.h at import.

The product path has no CPU fallback: if the library is missing, or a tensor is not on a
HIP device, the call raises.  PyTorch is used only for device memory and streams.
"""
import ctypes
import functools
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_void_p

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libsaicv_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(HERE), 'include', 'saicv_hip.h')

_SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'long long': ctypes.c_longlong, 'unsigned int': ctypes.c_uint,
            'unsigned long long': ctypes.c_ulonglong, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float,
            'double': ctypes.c_double}
_POINTEES = set(_SCALARS) | {'void', 'unsigned char', 'uint8_t', 'int32_t'}
_KEYWORDS = {w for t in _POINTEES | {'const', 'char', 'short', 'struct'} for w in t.split()}
_DECLARATOR = re.compile(r'(?:const\s+)?([A-Za-z_][\w ]*?)\s*(\**)\s*(\w+)(?:\[(\d+)\])?')


@functools.lru_cache(maxsize=None)
def struct_ptr(cls):
    """argtype of a `const saicv_x*` parameter: byref() of that struct and no other (a host descriptor), or None / an address
    (a device array of them)."""
    typed = POINTER(cls)

    class StructPtr:
        struct = cls

        @staticmethod
        def from_param(value):
            return c_void_p(value) if value is None or isinstance(value, int) else typed.from_param(value)
    return StructPtr


def _ctype(base, stars, structs, opaque, text):
    base = ' '.join(base.split())
    if not stars:
        if base in _SCALARS:
            return _SCALARS[base]
        if base in structs:
            return structs[base]
    elif base == 'char' and stars == '*':
        return c_char_p
    elif base in structs and stars == '*':
        return struct_ptr(structs[base])
    elif base in _POINTEES or base in opaque:
        return c_void_p
    raise ValueError(f'saicv_hip.h: unknown type {base + stars!r} in {text!r}')


def _declarator(text):
    m = _DECLARATOR.fullmatch(text.strip())
    if not m or m.group(3) in _KEYWORDS:          # `long long` without a name must not read as a `long` called long
        raise ValueError(f'saicv_hip.h: cannot split {text!r}')
    return m.groups()


def parse_header(text):
    """-> (constants {'SAICV_X': n}, structs {'saicv_x': Structure}, signatures {'saicv_f': (restype, argtypes)}).
    Reads `#define SAICV_X n`, `typedef struct ... { ... } name;` and `ret saicv_name(params);`; anything else raises."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#\s*ifdef\s+__cplusplus\b.*?^[ \t]*#\s*endif[^\n]*$', ' ', text, flags=re.S | re.M)
    constants = {k: int(v, 0) for k, v in re.findall(r'^[ \t]*#\s*define\s+(SAICV_\w+)\s+(-?\w+)[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#[^\n]*$', ' ', text, flags=re.M)
    opaque = set()
    for tag, name in re.findall(r'\btypedef\s+struct\s+(\w+)\s+(\w+)\s*;', text):
        if tag != name:
            raise ValueError(f'saicv_hip.h: opaque typedef {tag!r} is named {name!r}')
        opaque.add(name)
    text = re.sub(r'\btypedef\s+struct\s+\w+\s+\w+\s*;', ' ', text)
    structs = {}

    def struct(m):
        name, fields = m.group(2), []
        for stmt in filter(None, (s.strip() for s in m.group(1).split(';'))):
            first, *more = stmt.split(',')
            base, stars, field, count = _declarator(first)
            if stars and more:
                raise ValueError(f'saicv_hip.h: one pointer member per statement, got {stmt!r}')
            ct = _ctype(base, stars, structs, opaque, stmt)
            fields.append((field, ct * int(count) if count else ct))
            for extra in more:
                if not re.fullmatch(r'\s*\w+\s*', extra):
                    raise ValueError(f'saicv_hip.h: cannot split {stmt!r}')
                fields.append((extra.strip(), ct))
        structs[name] = type(''.join(w.capitalize() for w in name.split('_')[1:]), (Structure,),
                             {'_fields_': fields, '__doc__': f'{name} (include/saicv_hip.h)'})
        return ' '
    text = re.sub(r'\btypedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', struct, text)
    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(';'))):
        m = re.fullmatch(r'([^()]+)\(([^()]*)\)', stmt)
        if not m:
            raise ValueError(f'saicv_hip.h: cannot split {stmt!r}')
        base, stars, name, count = _declarator(m.group(1))
        params = [] if m.group(2).strip() == 'void' else [_declarator(p) for p in m.group(2).split(',')]
        if count or not name.startswith('saicv_') or name in signatures or any(p[3] for p in params):
            raise ValueError(f'saicv_hip.h: cannot bind {stmt!r}')
        signatures[name] = (_ctype(base, stars, structs, opaque, stmt), [_ctype(b, s, structs, opaque, stmt) for b, s, _, _ in params])
    return constants, structs, signatures


# A signature is written in the header and in the definition under csrc/: the compiler checks the two against each other,
# and this table is the header as parsed -- name -> (restype, argtypes)
_CONSTANTS, _STRUCTS, SIGNATURES = parse_header(open(HEADER_PATH).read())
globals().update({k[len('SAICV_'):]: v for k, v in _CONSTANTS.items()})      # BF16, F32, PLAN_*, ROUTE_*
globals().update({cls.__name__: cls for cls in _STRUCTS.values()})           # ConvDesc, AttnDesc, DgradFuse, PlanQuery, Plan, ...

_lib = None


def available():
    return os.path.exists(LIB_PATH)


def lib():
    """Loads the library (once).  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: run `python __graft_entry__.py` (build()) first. '
                'The MI355X HIP extension is required; there is no CPU/eager fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().saicv_last_error_string()
        raise RuntimeError(f'libsaicv_hip {what} failed ({rc}): {msg.decode() if msg else "?"}')


def dtype_code(dt):
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float32:
        return F32
    raise TypeError(f'saicv kernels support bfloat16 and float32, got {dt}')


def epc(dt):
    return 8 if dt == torch.bfloat16 else 4


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('saicv HIP kernels need tensors on an MI355X device (got a CPU tensor); '
                               'there is no CPU fallback in the product path')
