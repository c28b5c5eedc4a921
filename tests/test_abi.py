"""CPU-only: the C-ABI library builds, loads, and exports every symbol include/t2amd.h declares; and the ctypes binding
(tacotron2_subword_amd/_lib.py) says what the header says: every struct's size, field offsets, field sizes and field count,
every mirrored constant, and every prototype.  The header side comes from the host C compiler, not from a second reading of
the header: a C program generated from the ctypes classes includes t2amd.h and prints sizeof / offsetof."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "t2amd.h")


def _header_text():
    """t2amd.h without comments."""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(t2_[a-z0-9_]+)\s*\(", _header_text())))


def test_library_exports_every_declared_symbol():
    from tacotron2_subword_amd import build
    path = build.build()
    lib = ctypes.CDLL(path)
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), n


def test_binding_lists_every_declared_symbol():
    from tacotron2_subword_amd import _lib
    assert sorted(_lib.EXPORTS) == _declared()


def test_layout_query_and_error_path_without_gpu():
    from tacotron2_subword_amd import _lib as L
    from oracle import tacotron2_oracle as O
    hp = O.default_hparams()
    dims = L.dims_from_hparams(hp)
    lay = L.decoder_layout(dims, 64, 400, 100, 60)
    assert lay.total_floats * 4 < 8 << 30
    assert lay.din % 4 == 0 and lay.dout % 4 == 0
    bad = L.dims_from_hparams(dict(hp, prenet_dim=100))
    out = L.DecoderLayout()
    rc = L.lib().t2_decoder_layout_query(ctypes.byref(bad), 2, 3, 4, 5, ctypes.byref(out))
    assert rc != 0 and b"multiples of 64" in L.lib().t2_last_error()


def test_no_cpu_fallback():
    """CPU tensors are refused loudly."""
    import torch
    from tacotron2_subword_amd import _lib as L
    with pytest.raises(RuntimeError):
        L.ptr(torch.zeros(4))


# ------------------------------------------------------------------------------------------------------------------
# header against binding
# ------------------------------------------------------------------------------------------------------------------
def _key(name):
    """t2_decoder_fwd_args and DecoderFwdArgs pair up: no t2_, no underscores, no case."""
    return re.sub(r"^t2_", "", name).replace("_", "").lower()


def _header_structs():
    """{typedef name: number of fields} of every `typedef struct` of the header.  A declaration `T a, *b, c[2];` holds three."""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _header_text(), flags=re.S):
        tag, body, name = m.groups()
        assert tag == name and "{" not in body, name
        out[name] = sum(d.count(",") + 1 for d in body.split(";") if d.strip())
    return out


def _binding_structs():
    from tacotron2_subword_amd import _lib
    return {n: c for n, c in vars(_lib).items()
            if inspect.isclass(c) and issubclass(c, ctypes.Structure) and c.__module__ == _lib.__name__ and n == c.__name__}


def _constants():
    """(the header's name, the value the binding carries) for every constant _lib.py mirrors."""
    from tacotron2_subword_amd import _lib as L
    pairs = [("T2_ABI_VERSION", L.ABI_VERSION), ("T2_ATTN_SMA", L.ATTN_SMA), ("T2_ATTN_LSA", L.ATTN_LSA), ("T2_ATTN_FWD2", L.ATTN_FWD2),
             ("T2_ATTN_GMM", L.ATTN_GMM), ("T2_ATTN_DCA", L.ATTN_DCA)]
    pairs += [("T2_SITE_" + k, v) for k, v in L.SITE.items()]
    pairs += [("T2_CHAIN_" + k.upper(), v) for k, v in L.CHAIN_KINDS.items()]
    pairs += [("T2_CHAIN_PARTS", L.CHAIN_PARTS), ("T2_CHAIN_REFUSE_SHAPE", L.CHAIN_REFUSE_SHAPE),
              ("T2_CHAIN_REFUSE_NO_SAVED_TILES", L.CHAIN_REFUSE_NO_SAVED_TILES)]
    pairs += [("T2_PASS_" + k.upper(), v) for k, v in L.PASS_KINDS.items()]
    pairs += [("T2_PASS_MAX_BOUNDS", L.PASS_MAX_BOUNDS), ("T2_VOCODER_TIME_TILE", L.VOCODER_TIME_TILE), ("T2_STFT_FRAME_TILE", L.STFT_FRAME_TILE),
              ("T2_STFT_POLAR", L.STFT_POLAR), ("T2_STFT_DENOISE", L.STFT_DENOISE),
              ("T2_WAVEGLOW_KERNELS", len(L.WAVEGLOW_KERNELS)), ("T2_WAVEGLOW_FORWARD_KERNELS", len(L.WAVEGLOW_FORWARD_KERNELS)),
              ("T2_WAVEGLOW_BACKWARD_KERNELS", len(L.WAVEGLOW_BACKWARD_KERNELS))]
    # (the header has no name for the two sentinels of t2_silence_plan_info.R: nothing to hold SILENCE_* against)
    return pairs


@pytest.fixture(scope="module")
def header_facts(tmp_path_factory):
    """What the host C compiler says about t2amd.h: {"S name": size, "O name.field": offset, "Z name.field": size, "C NAME": value}."""
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    assert cc, "no host C compiler (cc, gcc, clang or $CC): the binding cannot be held against include/t2amd.h"
    typedefs = {_key(n): n for n in _header_structs()}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "t2amd.h"', "int main(void) {"]
    for cname, cls in sorted(_binding_structs().items()):
        t = typedefs.get(_key(cname))
        if t is None:
            continue                                   # reported by test_every_struct_has_its_class
        lines.append(f'    printf("S {t} %zu\\n", sizeof({t}));')
        for field in cls._fields_:
            f = field[0]
            lines.append(f'    printf("O {t}.{f} %zu\\n", offsetof({t}, {f}));')
            lines.append(f'    printf("Z {t}.{f} %zu\\n", sizeof((({t}*)0)->{f}));')
    for name, _ in _constants():
        lines.append(f'    printf("C {name} %lld\\n", (long long)({name}));')
    lines += ["    return 0;", "}"]
    d = tmp_path_factory.mktemp("abi")
    src, exe = d / "abi_probe.c", d / "abi_probe"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, "a field or constant of _lib.py that include/t2amd.h does not have:\n" + r.stdout.decode(errors="replace")
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout.decode()
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}


def test_every_struct_has_its_class():
    typedefs = {_key(n): n for n in _header_structs()}
    classes = {_key(n): n for n in _binding_structs()}
    assert len(typedefs) == len(_header_structs()) and len(classes) == len(_binding_structs()), "two names fold onto one key"
    assert len(typedefs) >= 80
    assert sorted(typedefs[k] for k in typedefs.keys() - classes.keys()) == [], "typedefs of t2amd.h without a ctypes class"
    assert sorted(classes[k] for k in classes.keys() - typedefs.keys()) == [], "ctypes Structures of _lib.py without a typedef"


def test_struct_layouts_match_the_header(header_facts):
    counts = _header_structs()
    typedefs = {_key(n): n for n in counts}
    bad = []
    for cname, cls in sorted(_binding_structs().items()):
        t = typedefs.get(_key(cname))
        if t is None:
            continue
        if ctypes.sizeof(cls) != header_facts[f"S {t}"]:
            bad.append(f"{cname}: {ctypes.sizeof(cls)} bytes, {t} has {header_facts[f'S {t}']}")
        if len(cls._fields_) != counts[t]:
            bad.append(f"{cname}: {len(cls._fields_)} fields, {t} has {counts[t]}")
        for field in cls._fields_:
            d = getattr(cls, field[0])
            if (d.offset, d.size) != (header_facts[f"O {t}.{field[0]}"], header_facts[f"Z {t}.{field[0]}"]):
                bad.append(f"{cname}.{field[0]}: offset {d.offset} size {d.size}, {t} has offset {header_facts[f'O {t}.{field[0]}']} "
                           f"size {header_facts[f'Z {t}.{field[0]}']}")
    assert bad == []


def test_constants_match_the_header(header_facts):
    bad = [f"{name}: _lib.py has {value}, t2amd.h {header_facts['C ' + name]}" for name, value in _constants() if header_facts["C " + name] != value]
    assert bad == []


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def _prototypes():
    """{function: (return type, [parameter types])} of every declaration of the header, types as "base" + one "*" per level
    ("const" dropped).  What is left of the header once comments, preprocessor lines, struct bodies and enums are gone must be
    function declarations and nothing else: a statement this does not understand is an error, not a skip."""
    text = re.sub(r"^\s*#.*$", "", _header_text(), flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"\benum\s*\{.*?\}\s*;", "", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)

    def typ(s, named):
        s = re.sub(r"\bconst\b", " ", s).replace("*", " * ").split()
        if named and len(s) > 1 and s[-1] != "*":
            s = s[:-1]                                  # the parameter's name
        assert s and re.fullmatch(r"\w+", s[0]) and all(x == "*" for x in s[1:]), s
        return s[0] + "*" * (len(s) - 1)

    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):                           # (the closing brace of extern "C")
            continue
        m = re.fullmatch(r"(.+?)\b(t2_\w+) ?\((.*)\)", stmt)
        assert m, f"t2amd.h: not a function declaration: {stmt!r}"
        ret, name, params = m.groups()
        assert name not in out, name
        params = [] if params.strip() == "void" else [typ(p, True) for p in params.split(",")]
        out[name] = (typ(ret, False), params)
    return out


def _wanted(ctype, structs):
    """What a C type asks of the ctypes type in its place: ("is", type) or ("pointer",)."""
    if ctype in _SCALARS:
        return ("is", _SCALARS[ctype])
    assert ctype.endswith("*"), ctype
    base = ctype.rstrip("*")
    if base.startswith("t2_") and ctype == base + "*":
        return ("is", ctypes.POINTER(structs[_key(base)]))
    return ("pointer",)


def _meets(want, got):
    if want[0] == "is":
        return got is want[1]
    return got in (ctypes.c_void_p, ctypes.c_char_p) or (inspect.isclass(got) and issubclass(got, ctypes._Pointer))


def test_prototypes_match_the_header():
    from tacotron2_subword_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.EXPORTS)
    structs = {_key(n): c for n, c in _binding_structs().items()}
    lib = _lib.lib()
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        fn = getattr(lib, name)
        if not _meets(_wanted(ret, structs), fn.restype):
            bad.append(f"{name}: returns {ret}, restype is {fn.restype}")
        if fn.argtypes is None:
            if any(p != "int" for p in params):
                bad.append(f"{name}({', '.join(params)}): no argtypes, and not every parameter is an int")
            continue
        if len(fn.argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters, {len(fn.argtypes)} argtypes")
            continue
        for i, (p, got) in enumerate(zip(params, fn.argtypes)):
            if not _meets(_wanted(p, structs), got):
                bad.append(f"{name}: parameter {i} is {p}, argtypes has {got.__name__}")
    assert bad == []
