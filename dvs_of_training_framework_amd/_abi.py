"""Reader of include/dvsof.h: the ctypes signatures, Structures and integer
constants of the C ABI are DERIVED from the header, the one place they are
written down.  Pure Python (re, ctypes, numpy), no compiler.

It understands the C subset the header uses and nothing else:
  functions  ``ret name(params);`` -- scalars, pointers of any depth, const
             anywhere, ``type name[]``, ``(void)``
  structs    ``typedef struct { ... } name_t;`` -- scalar, pointer, ``int B, H, W;``,
             fixed arrays, a nested struct by typedef name
  constants  ``#define DVSOF_NAME <integer>`` and ``enum { NAME = <integer>, ... }``
Anything else raises AbiError with the header line number; nothing is skipped.

Type rule, the same for every function: a scalar is its ctypes twin, ``char *``
is c_char_p, a pointer to a struct typedef is POINTER(that Structure) -- one that
also converts a plain address, because the record structs live in tensors and
arrive as ``tensor.data_ptr()`` --, EVERY other pointer is c_void_p.  Callers
pass ``tensor.data_ptr()`` integers for device pointers and ``byref(...)`` or
ctypes arrays for host out-parameters and tables; c_void_p takes all three.
Host out-parameters (``int *n_marks``, ``size_t *n``) are therefore NOT checked
to be POINTER(c_int) / POINTER(c_size_t): the price of a rule that needs no
per-function knowledge.  Struct fields: a pointer is c_void_p, a nested struct
its class, natural alignment (the ctypes default, which is the C compiler's).
"""
import ctypes
import re
from pathlib import Path

import numpy as np

HEADER_PATH = Path(__file__).resolve().parent.parent / 'include' / 'dvsof.h'
# Extension headers, read after dvsof.h with its struct types known: their entry points are
# tables of their own (EXTENSION_FUNCTIONS), beside the recorded one of dvsof.h (FUNCTIONS)
EXTENSION_PATHS = (HEADER_PATH.with_name('dvsof_contrast.h'),)
# A later extension with a table of its own again (CONTRAST_MULTI_FUNCTIONS): the table of
# dvsof_contrast.h is recorded as exactly its three names and stays that
CONTRAST_MULTI_PATH = HEADER_PATH.with_name('dvsof_contrast_multi.h')
# And one more (IWE_MULTI_FUNCTIONS): the validation side of the same options
IWE_MULTI_PATH = HEADER_PATH.with_name('dvsof_iwe_multi.h')
# And the loss of a run without frames (LOSS_FRAMELESS_FUNCTIONS)
LOSS_FRAMELESS_PATH = HEADER_PATH.with_name('dvsof_loss_frameless.h')
# And the contrast term on every flow scale (CONTRAST_PYRAMID_FUNCTIONS), the one extension with
# structs of its own (CONTRAST_PYRAMID_STRUCTS: the level table, passed by value)
CONTRAST_PYRAMID_PATH = HEADER_PATH.with_name('dvsof_contrast_pyramid.h')
# And the average-timestamp term (AVG_TIMESTAMP_FUNCTIONS), functions only
AVG_TIMESTAMP_PATH = HEADER_PATH.with_name('dvsof_avg_timestamp.h')
# And that term on every flow scale (AVG_TIMESTAMP_PYRAMID_FUNCTIONS): functions only, which take
# the level table of dvsof_contrast_pyramid.h
AVG_TIMESTAMP_PYRAMID_PATH = HEADER_PATH.with_name('dvsof_avg_timestamp_pyramid.h')
# And the two events-only terms on the encoded event columns (EVENT_TERMS_ENCODED_FUNCTIONS):
# functions only, the twins of calls of the four headers before it
EVENT_TERMS_ENCODED_PATH = HEADER_PATH.with_name('dvsof_event_terms_encoded.h')
# And the average-timestamp images of the validation metric (IWE_AVG_TIMESTAMP_FUNCTIONS), functions only
IWE_AVG_TIMESTAMP_PATH = HEADER_PATH.with_name('dvsof_iwe_avg_timestamp.h')

_SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'size_t': ctypes.c_size_t, 'unsigned long long': ctypes.c_ulonglong}
for _n in (8, 16, 32, 64):
    _SCALARS[f'int{_n}_t'] = getattr(ctypes, f'c_int{_n}')
    _SCALARS[f'uint{_n}_t'] = getattr(ctypes, f'c_uint{_n}')
_INT = r'[-+]?(?:0[xX][0-9a-fA-F]+|\d+)'


class AbiError(ValueError):
    pass


def _struct_pointer(struct):
    """POINTER(struct) that converts an int (the address of records in a tensor) too."""
    base = ctypes.POINTER(struct)

    def from_param(cls, v):
        return ctypes.c_void_p(v) if isinstance(v, int) else base.from_param(v)
    return type(base.__name__, (base,), {'from_param': classmethod(from_param)})


class Abi:
    """functions {name: (restype, argtypes)}, structs {name: Structure class},
    constants {name: int} of one header text.  ``base``: the Abi of a header this
    one includes, whose struct types it may name; ``name`` goes into the errors."""

    def __init__(self, text, base=None, name='dvsof.h'):
        self.functions, self.structs, self.constants, self._pointers = {}, {}, {}, {}
        self._name = name
        if base is not None:
            self.structs, self._pointers = dict(base.structs), dict(base._pointers)
        self._text = text = self._preprocess(text)
        depth = start = 0
        for m in re.finditer(r'[{};]', text):       # statements end at a ';' outside braces
            depth += {'{': 1, '}': -1, ';': 0}[m.group()]
            if m.group() == ';' and depth == 0:
                self._statement(start, text[start:m.start()])
                start = m.end()
        if text[start:].strip():
            self._fail(start, 'declaration without a terminating ;')

    def _fail(self, pos, why):
        pos += len(self._text[pos:]) - len(self._text[pos:].lstrip())
        raise AbiError(f'{self._name} line {self._text.count(chr(10), 0, pos) + 1}: {why}')

    def _preprocess(self, text):
        """Comments and preprocessor lines -> blanks (line numbers stay);
        #define NAME <integer> -> constants; the extern "C" wrapper goes."""
        text = re.sub(r'/\*.*?\*/', lambda m: re.sub(r'[^\n]', ' ', m.group()), text, flags=re.S)
        self._text, lines, cxx, pos = text, text.split('\n'), [], 0
        for i, line in enumerate(lines):
            word = line.split()
            if word and word[0].startswith('#'):
                if word[0] in ('#if', '#ifdef', '#ifndef'):
                    cxx.append('__cplusplus' in line)
                elif word[0] == '#endif':
                    cxx.pop()
                elif word[0] == '#define' and len(word) > 2:
                    if not re.fullmatch(_INT, ' '.join(word[2:])):
                        self._fail(pos, f'#define {word[1]} is not an integer')
                    self.constants[word[1]] = int(word[2], 0)
                elif word[0] not in ('#define', '#include'):
                    self._fail(pos, f'unknown directive {word[0]}')
                lines[i] = ''
            elif any(cxx):
                lines[i] = ''
            pos += len(line) + 1
        return '\n'.join(lines)

    def _statement(self, pos, s):
        if m := re.fullmatch(r'\s*typedef\s+struct\s*\{(.*)\}\s*(\w+)\s*', s, re.S):
            fields, body, at = [], m.group(1), pos + m.start(1)
            for f in re.finditer(r'[^;]*;', body):
                first, *more = f.group()[:-1].split(',')
                ctype, name, base = self._declarator(at + f.start(), first, field=True)
                fields.append((name, ctype))
                for d in more:                      # int B, H, W;
                    ctype, name, _ = self._declarator(at + f.start(), f'{base} {d}', field=True)
                    fields.append((name, ctype))
            if body[body.rfind(';') + 1:].strip():
                self._fail(at + body.rfind(';') + 1, 'field without a terminating ;')
            self.structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {'_fields_': fields})
            self._pointers[m.group(2)] = _struct_pointer(self.structs[m.group(2)])
        elif m := re.fullmatch(r'\s*enum\s*\{(.*)\}\s*', s, re.S):
            for e in re.finditer(r'[^,]+', m.group(1)):
                if not e.group().strip():
                    continue
                if not (v := re.fullmatch(rf'\s*(\w+)\s*=\s*({_INT})\s*', e.group())):
                    self._fail(pos + m.start(1) + e.start(), 'enum member without an explicit integer value')
                self.constants[v.group(1)] = int(v.group(2), 0)
        elif m := re.fullmatch(r'([^(){}]*)\((.*)\)\s*', s, re.S):
            restype, name, _ = self._declarator(pos, m.group(1), ret=True)
            params = [] if m.group(2).strip() == 'void' else list(re.finditer(r'[^,]+', m.group(2)))
            self.functions[name] = (restype, [self._declarator(pos + m.start(2) + p.start(), p.group())[0]
                                              for p in params])
        else:
            self._fail(pos, 'not a function declaration, typedef struct or enum')

    def _declarator(self, pos, s, field=False, ret=False):
        """'const float *const *levels' -> (ctypes type, name, base type name)."""
        tok = [t for t in re.findall(r'\w+|\[\w*\]|\S', s) if t != 'const']
        array = tok.pop()[1:-1] if tok and tok[-1][0] == '[' else None
        name = tok.pop() if tok else ''
        stars, base = tok.count('*'), ' '.join(t for t in tok if t != '*')
        if not re.fullmatch(r'[A-Za-z_]\w*', name) or not re.fullmatch(r'[\w ]*', base) \
                or (array is not None and (ret or bool(re.fullmatch(_INT, array)) != field)):
            self._fail(pos, f'unsupported declarator "{" ".join(s.split())}"')
        if base not in _SCALARS and base not in self.structs \
                and not (base == 'void' and (stars or ret)) and not (base == 'char' and stars):
            self._fail(pos, f'unknown type "{base}" in "{" ".join(s.split())}"')
        if array is not None and not field:
            stars += 1                              # type name[] is a pointer parameter
        if stars == 0:
            ctype = None if base == 'void' else _SCALARS.get(base) or self.structs[base]
        elif stars == 1 and base in self.structs and not field:
            ctype = self._pointers[base]
        else:
            ctype = ctypes.c_char_p if (stars == 1 and base == 'char' and not field) else ctypes.c_void_p
        if field and array is not None:
            ctype = ctype * int(array, 0)
        return ctype, name, base


def dtype_of(struct):
    """numpy dtype of a record struct that travels through tensors: every field a
    scalar or a pointer (-> '<u8'), offsets and itemsize those of the Structure."""
    cls = STRUCTS[struct] if isinstance(struct, str) else struct
    names, formats = [], []
    for name, ctype in cls._fields_:
        if not issubclass(ctype, ctypes._SimpleCData):
            raise TypeError(f'{cls.__name__}.{name} is neither a scalar nor a pointer')
        names.append(name)
        formats.append('<u8' if ctype is ctypes.c_void_p else np.dtype(ctype))
    return np.dtype({'names': names, 'formats': formats, 'itemsize': ctypes.sizeof(cls),
                     'offsets': [getattr(cls, n).offset for n in names]})


_header = Abi(HEADER_PATH.read_text())
FUNCTIONS, STRUCTS, CONSTANTS = _header.functions, _header.structs, _header.constants
EXTENSION_FUNCTIONS = {}


def _read_extension(path, taken, base=None):
    """The functions of one extension header; ``taken``: the names it must not repeat;
    ``base``: the Abi of the header it includes, whose struct types it may name (dvsof.h)."""
    base = _header if base is None else base
    ext = Abi(path.read_text(), base=base, name=path.name)
    clash = set(ext.functions) & set(taken)
    if clash or ext.constants or set(ext.structs) != set(base.structs):
        raise AbiError(f'{path.name}: an extension header declares new functions only '
                       f'({sorted(clash) or "constants or structs found"})')
    return ext.functions


for _path in EXTENSION_PATHS:
    EXTENSION_FUNCTIONS.update(_read_extension(_path, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS)))
CONTRAST_MULTI_FUNCTIONS = _read_extension(CONTRAST_MULTI_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS))
IWE_MULTI_FUNCTIONS = _read_extension(IWE_MULTI_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS)
                                     | set(CONTRAST_MULTI_FUNCTIONS))
LOSS_FRAMELESS_FUNCTIONS = _read_extension(LOSS_FRAMELESS_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS)
                                          | set(CONTRAST_MULTI_FUNCTIONS) | set(IWE_MULTI_FUNCTIONS))


def _read_struct_extension(path, taken):
    """An extension header that also declares structs of its own (a table passed by value):
    -> (functions, {name: Structure} of the new structs).  STRUCTS stays that of dvsof.h."""
    ext = Abi(path.read_text(), base=_header, name=path.name)
    clash = set(ext.functions) & set(taken)
    if clash or ext.constants or not set(STRUCTS) <= set(ext.structs):
        raise AbiError(f'{path.name}: an extension header declares new functions and structs only '
                       f'({sorted(clash) or "constants found"})')
    _struct_headers[path] = ext
    return ext.functions, {k: v for k, v in ext.structs.items() if k not in STRUCTS}


_struct_headers = {}    # {path: Abi} of the extension headers with structs, for those that include them
CONTRAST_PYRAMID_FUNCTIONS, CONTRAST_PYRAMID_STRUCTS = _read_struct_extension(
    CONTRAST_PYRAMID_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS) | set(CONTRAST_MULTI_FUNCTIONS)
    | set(IWE_MULTI_FUNCTIONS) | set(LOSS_FRAMELESS_FUNCTIONS))
AVG_TIMESTAMP_FUNCTIONS = _read_extension(
    AVG_TIMESTAMP_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS) | set(CONTRAST_MULTI_FUNCTIONS)
    | set(IWE_MULTI_FUNCTIONS) | set(LOSS_FRAMELESS_FUNCTIONS) | set(CONTRAST_PYRAMID_FUNCTIONS))
AVG_TIMESTAMP_PYRAMID_FUNCTIONS = _read_extension(
    AVG_TIMESTAMP_PYRAMID_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS) | set(CONTRAST_MULTI_FUNCTIONS)
    | set(IWE_MULTI_FUNCTIONS) | set(LOSS_FRAMELESS_FUNCTIONS) | set(CONTRAST_PYRAMID_FUNCTIONS)
    | set(AVG_TIMESTAMP_FUNCTIONS), base=_struct_headers[CONTRAST_PYRAMID_PATH])
EVENT_TERMS_ENCODED_FUNCTIONS = _read_extension(
    EVENT_TERMS_ENCODED_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS) | set(CONTRAST_MULTI_FUNCTIONS)
    | set(IWE_MULTI_FUNCTIONS) | set(LOSS_FRAMELESS_FUNCTIONS) | set(CONTRAST_PYRAMID_FUNCTIONS)
    | set(AVG_TIMESTAMP_FUNCTIONS) | set(AVG_TIMESTAMP_PYRAMID_FUNCTIONS),
    base=_struct_headers[CONTRAST_PYRAMID_PATH])
IWE_AVG_TIMESTAMP_FUNCTIONS = _read_extension(
    IWE_AVG_TIMESTAMP_PATH, set(FUNCTIONS) | set(EXTENSION_FUNCTIONS) | set(CONTRAST_MULTI_FUNCTIONS)
    | set(IWE_MULTI_FUNCTIONS) | set(LOSS_FRAMELESS_FUNCTIONS) | set(CONTRAST_PYRAMID_FUNCTIONS)
    | set(AVG_TIMESTAMP_FUNCTIONS) | set(AVG_TIMESTAMP_PYRAMID_FUNCTIONS) | set(EVENT_TERMS_ENCODED_FUNCTIONS))
