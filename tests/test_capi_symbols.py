"""CPU-side checks of the drop-in boundary: the shared library loads and exports exactly the entry
points include/aim_kernels.h declares (no compute is launched without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "aim_kernels.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(aim_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_binding_table():
    from aim_amd.lib import SIGNATURES
    assert _declared() == sorted(SIGNATURES)


def test_library_exports_every_declared_symbol():
    import aim_amd
    path = aim_amd.library_path()
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(path)
    for name in _declared():
        assert hasattr(lib, name), name
    from aim_amd.lib import ABI_VERSION
    assert aim_amd.load_library().aim_version() == ABI_VERSION


# ------------------------------------------------------------------ the header against the binding table, type by type -----
# An `int` / `int64_t` swap, a missing argument or a struct field the mirror lacks may still give right answers at small
# shapes (the value sits in a 64-bit register or stack slot either way), so the names above are not enough.
def _header():
    text = open(os.path.join(ROOT, "include", "aim_kernels.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _c_kind(decl):
    """one C parameter or field declaration without its name's array part -> 'P' | 'I' | 'L' | 'F' (+ the pointed-to struct)"""
    if "*" in decl:
        m = re.search(r"\b(aim_\w+_args)\s*\*", decl)
        return "P", (m.group(1) if m else None)
    words = [w for w in decl.split() if w != "const"]
    base = {"int": "I", "int32_t": "I", "int64_t": "L", "float": "F"}.get(" ".join(words[:-1]))
    assert base, f"unknown C type in {decl!r}"
    return base, None


def _c_prototypes():
    """name -> (return type, [kind of every parameter]) for every prototype of the header"""
    out = {}
    for ret, name, params in re.findall(r"\b(int64_t|int|const\s+char\s*\*)\s*(aim_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        params = params.strip()
        out[name] = (re.sub(r"\s+", " ", ret).replace(" *", "*"),
                     [] if params in ("", "void") else [_c_kind(p.strip()) for p in params.split(",")])
    return out


def _c_structs():
    """struct name -> [(field, kind, array length or 0)] in declaration order"""
    out = {}
    for name, body, name2 in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _header(), flags=re.S):
        assert name == name2
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            first, *more = [d.strip() for d in decl.split(",")]
            m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[(\d+)\])?", first, flags=re.S)
            kind = _c_kind(m.group(1) + " x")[0]
            fields.append((m.group(2), kind, int(m.group(3) or 0)))
            for d in more:                          # `int32_t lda, ldw`: further plain names of the same type
                assert re.fullmatch(r"\w+", d) and kind != "P", decl
                fields.append((d, kind, 0))
        out[name] = fields
    return out


def _ct_kind(t):
    """a ctypes type -> the same alphabet"""
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "P", t._type_
    if t is ctypes.c_void_p or t is ctypes.c_char_p:
        return "P", None
    for kind, group in (("I", (ctypes.c_int, ctypes.c_int32)), ("L", (ctypes.c_int64,)), ("F", (ctypes.c_float,))):
        if t in group:
            return kind, None
    raise AssertionError(f"unknown ctypes type {t}")


ARG_STRUCTS = {"aim_gemm_args": "GemmArgs", "aim_wgrad_ride_args": "WgradRideArgs", "aim_lowrank_args": "LowrankArgs"}


def _signature_mismatches(signatures, classes):
    """every disagreement between the header's prototypes and `signatures` (name -> argtypes); classes: C struct -> mirror"""
    bad, protos = [], _c_prototypes()
    if sorted(protos) != sorted(signatures):
        bad.append(f"names differ: {sorted(set(protos) ^ set(signatures))}")
    for name, (_, want) in protos.items():
        have = signatures.get(name)
        if have is None:
            continue
        if len(have) != len(want):
            bad.append(f"{name}: {len(want)} parameters in the header, {len(have)} in the table")
            continue
        for i, ((wk, wstruct), t) in enumerate(zip(want, have)):
            hk, hstruct = _ct_kind(t)
            if hk != wk:
                bad.append(f"{name} argument {i}: header {wk}, table {hk}")
            elif wstruct is not None and hstruct is not classes[wstruct]:
                bad.append(f"{name} argument {i}: header points to {wstruct}, table to {hstruct}")
    return bad


def _struct_mismatches(classes):
    bad, structs = [], _c_structs()
    for cname, cls in classes.items():
        want = structs[cname]
        have = []
        for fname, t in cls._fields_:
            n = 0
            if isinstance(t, type) and issubclass(t, ctypes.Array):
                t, n = t._type_, t._length_
            have.append((fname, _ct_kind(t)[0], n))
        if have != want:
            diff = [f"{w} != {h}" for w, h in zip(want, have) if w != h][:3]
            bad.append(f"{cname}: {len(want)} fields in the header, {len(have)} in the mirror; first differences: {diff}")
    return bad


def _mirrors():
    from aim_amd import lib as L
    return {c: getattr(L, p) for c, p in ARG_STRUCTS.items()}


def test_signatures_match_the_prototypes_argument_by_argument():
    from aim_amd.lib import SIGNATURES
    protos = _c_prototypes()
    assert sorted(protos) == _declared()                         # the prototype parser saw every declared entry point
    assert len(protos) >= 85
    assert not _signature_mismatches(SIGNATURES, _mirrors())
    # return types: the header's against the ones the loader sets
    import aim_amd
    path = aim_amd.library_path()
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    lib = aim_amd.load_library()
    for name, (ret, _) in protos.items():
        want = "const char*" if name == "aim_last_error" else "int64_t" if name.endswith("_bytes") else "int"
        assert ret == want, (name, ret)
        have = getattr(lib, name).restype
        assert have is {"const char*": ctypes.c_char_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}[ret], (name, have)


def test_structures_match_the_structs_field_by_field():
    structs = _c_structs()
    assert [len(structs[c]) for c in ARG_STRUCTS] == [39, 13, 19]
    assert sum(n == 3 for _, _, n in structs["aim_lowrank_args"]) == 7
    assert not _struct_mismatches(_mirrors())
    # the mirrors are as large as the C compiler makes them (natural alignment on both sides)
    for cname, cls in _mirrors().items():
        size = off = 0
        for _, kind, n in structs[cname]:
            w = {"P": 8, "L": 8, "I": 4, "F": 4}[kind]
            off = (off + w - 1) // w * w + w * max(n, 1)
        size = (off + 7) // 8 * 8
        assert ctypes.sizeof(cls) == size, (cname, ctypes.sizeof(cls), size)


def test_the_binding_check_sees_seeded_defects():
    from aim_amd import lib as L
    mirrors = _mirrors()
    # an int64_t stride bound as int
    sig = {k: list(v) for k, v in L.SIGNATURES.items()}
    assert sig["aim_add_bf16"][3] is L.L
    sig["aim_add_bf16"][3] = L.I
    bad = _signature_mismatches(sig, mirrors)
    assert len(bad) == 1 and bad[0].startswith("aim_add_bf16 argument 3"), bad
    # and the other way round
    sig = {k: list(v) for k, v in L.SIGNATURES.items()}
    sig["aim_add_bf16"][6] = L.L
    bad = _signature_mismatches(sig, mirrors)
    assert len(bad) == 1 and bad[0].startswith("aim_add_bf16 argument 6"), bad
    # a missing argument
    sig = {k: list(v) for k, v in L.SIGNATURES.items()}
    del sig["aim_embed_ln_bwd"][5]
    bad = _signature_mismatches(sig, mirrors)
    assert len(bad) == 1 and bad[0].startswith("aim_embed_ln_bwd: 22 parameters in the header, 21"), bad
    # the wrong structure behind an *_args pointer
    sig = {k: list(v) for k, v in L.SIGNATURES.items()}
    sig["aim_lowrank_fwd"][0] = ctypes.POINTER(L.GemmArgs)
    bad = _signature_mismatches(sig, mirrors)
    assert len(bad) == 1 and bad[0].startswith("aim_lowrank_fwd argument 0"), bad

    # a field of aim_gemm_args the mirror lacks; a field of the wrong width; two fields swapped
    def variant(fields):
        return dict(mirrors, aim_gemm_args=type("GemmArgsVariant", (ctypes.Structure,), {"_fields_": fields}))

    fields = list(L.GemmArgs._fields_)
    assert any(n == "row0" for n, _ in fields)
    bad = _struct_mismatches(variant([f for f in fields if f[0] != "row0"]))
    assert len(bad) == 1 and bad[0].startswith("aim_gemm_args: 39 fields in the header, 38"), bad
    bad = _struct_mismatches(variant([(n, ctypes.c_int32 if n == "strideA" else t) for n, t in fields]))
    assert len(bad) == 1 and "strideA" in bad[0], bad
    i = [n for n, _ in fields].index("ldv")
    bad = _struct_mismatches(variant(fields[:i] + [fields[i + 1], fields[i]] + fields[i + 2:]))
    assert len(bad) == 1 and "ldv" in bad[0], bad


def _rocm_clang():
    """the clang of the ROCm toolchain that the build's hipcc (HIPCC, default /opt/rocm/bin/hipcc as in csrc/Makefile) drives"""
    hipcc = os.path.realpath(os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc")
    root = os.path.dirname(os.path.dirname(hipcc))
    for rel in ("llvm/bin/clang", "lib/llvm/bin/clang"):
        p = os.path.join(root, rel)
        if os.path.exists(p):
            return p
    return None


def test_header_parses_as_plain_c99(tmp_path):
    import subprocess
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("no ROCm clang on this machine")
    src = tmp_path / "use_header.c"
    src.write_text('#include "aim_kernels.h"\nint aim_header_probe(void) { return (int)sizeof(aim_gemm_args) + AIM_ABI_VERSION; }\n')
    p = subprocess.run([clang, "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr


def test_missing_library_is_loud(monkeypatch):
    from aim_amd import lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setattr(L, "library_path", lambda: "/nonexistent/libaim_hip.so")
    with pytest.raises(L.LibraryNotBuilt):
        L.load_library()


def test_ops_refuse_cpu_tensors():
    import torch
    from aim_amd import ops
    a = torch.zeros((8, 8), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm(a, a, ops.EPI_BF16, torch.zeros((8, 8), dtype=torch.bfloat16))
