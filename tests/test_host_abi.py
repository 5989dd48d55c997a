"""CPU-side checks of the host driver's C boundary: include/spartan_host.h declares every spz_* entry point once; the library exports each of
them (host_capi.cc does not compile otherwise), the one table spartan_amd/prover.py binds from agrees with the header type by type, the header
is C99, and the hand-written Rust declarations of the coarse binding name declared functions with the right number of parameters."""
import ctypes, importlib.util, os, re, shutil, subprocess
import pytest
from tests.helpers import ROOT

HEADER = os.path.join(ROOT, "include", "spartan_host.h")
RETURNS = r"const char\*|void\*|sp_ctx\*|long long|double|size_t|void|int"
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
           "long long": ctypes.c_longlong, "void": None}
POINTERS = (ctypes.c_void_p, ctypes.c_char_p)


@pytest.fixture(scope="module")
def protos():
    spec = importlib.util.spec_from_file_location("gen_gpu_rs", os.path.join(ROOT, "rust_shim", "gen_gpu_rs.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    return {name: (ret, params) for name, ret, params in gen.parse_header(HEADER, prefix="spz_", returns=RETURNS)}


def _function_pointer_types():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"typedef\s+\w+\s*\(\s*\*\s*(\w+)\s*\)", src))


def _matches(ctype, bound, fn_types):
    """does the ctypes type `bound` stand for the C type `ctype`?"""
    if "*" in ctype or ctype in fn_types:
        return bound in POINTERS and (bound is ctypes.c_void_p or ctype == "const char*")   # c_char_p only where C says const char*
    return ctype in SCALARS and bound is SCALARS[ctype]


def test_header_declares_what_the_library_exports_and_the_table_binds(protos):
    from spartan_amd import prover
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    named = set(re.findall(r"\b(spz_\w+)\s*\(", src))          # every spz_* name followed by "(": the parser missed none of them
    assert named == set(protos) and len(protos) >= 85
    for name in protos:
        assert hasattr(prover.H, name), f"{name} declared in spartan_host.h but not exported"
    assert set(prover.SIGNATURES) == set(protos)


def test_table_matches_the_header_type_by_type(protos):
    from spartan_amd import prover
    fn_types = _function_pointer_types()
    assert fn_types == {"spz_commit_gather_fn"}
    for name, (ret, params) in protos.items():
        restype, argtypes = prover.SIGNATURES[name]
        assert _matches(ret, restype, fn_types), (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for (ctype, arg), bound in zip(params, argtypes):
            assert _matches(ctype, bound, fn_types), (name, arg, ctype, bound)
        f = getattr(prover.H, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name   # ... and the table is what was applied


def test_header_is_c99():
    clang = os.environ.get("CLANG") or "/opt/rocm/lib/llvm/bin/clang"
    if not (os.path.exists(clang) or shutil.which(clang)):
        pytest.skip(f"{clang}: the clang that ships with ROCm is not installed")
    r = subprocess.run([clang, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]


def test_hand_written_rust_declarations_match_the_header(protos):
    """rust_shim/src/gpu_tail.rs.in declares the spz_* functions of the coarse binding by hand: each names a declared function and takes as many
    parameters as the header gives it, pointers where the header has pointers"""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust_shim", "src", "gpu_tail.rs.in")).read())
    decls = re.findall(r"pub fn (spz_\w+)\s*\((.*?)\)\s*(?:->\s*([^;]+))?;", src, flags=re.S)
    assert {d[0] for d in decls} >= {"spz_snark_prove_t", "spz_nizk_prove_t", "spz_proof_bytes", "spz_proof_free", "spz_transcript_probe"}
    for name, args, ret in decls:
        assert name in protos, f"{name} declared in gpu_tail.rs.in but not in spartan_host.h"
        cret, params = protos[name]
        rust = [a.split(":", 1)[1].strip() for a in args.split(",") if a.strip()]
        assert len(rust) == len(params), (name, len(rust), len(params))
        for (ctype, arg), rt in zip(params, rust):
            assert rt.startswith("*") == ("*" in ctype), (name, arg, ctype, rt)
        assert bool(ret.strip()) == (cret != "void"), (name, cret, ret)
    for name in set(re.findall(r"\b(spz_\w+)\s*\(", src)):      # and every call names one of them
        assert name in {d[0] for d in decls}, name
