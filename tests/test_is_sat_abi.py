"""CPU-side checks of the device satisfiability check's boundary (sp_r1cs_check, Instance::is_sat): the entry point is declared, exported and
bound; it refuses null handles before it touches a device; the Rust seam and INTEGRATION.md name it."""
import ctypes, os, re
from tests.helpers import ROOT


def test_sp_r1cs_check_is_declared_exported_and_bound():
    from spartan_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spartan_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+sp_r1cs_check\s*\(([^;]*)\)\s*;", hdr)
    assert m, "sp_r1cs_check is not declared in include/spartan_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["sp_ctx* ctx", "const sp_sparse* A", "const sp_sparse* B", "const sp_sparse* C", "const sp_table* z", "uint64_t* violated",
                    "uint64_t* first_row", "uint64_t* rows_out", "size_t rows_cap"]
    assert hasattr(capi.lib, "sp_r1cs_check") and "sp_r1cs_check" in capi.SYMBOLS
    gpu_rs = open(os.path.join(ROOT, "rust_shim", "src", "gpu.rs")).read()
    assert ("pub fn sp_r1cs_check(ctx: *mut sp_ctx, A: *const sp_sparse, B: *const sp_sparse, C: *const sp_sparse, z: *const sp_table, "
            "violated: *mut u64, first_row: *mut u64, rows_out: *mut u64, rows_cap: usize) -> i32;") in gpu_rs


def test_sp_r1cs_check_refuses_null_handles_without_a_device():
    """SP_EINVAL (-1) for every null handle and null result pointer: decided before any HIP call, so it holds on a machine without a GPU"""
    from spartan_amd import capi
    L = capi.lib
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    v, f = ctypes.c_uint64(7), ctypes.c_uint64(7)
    fake = ctypes.create_string_buffer(256)   # never dereferenced: a null argument is found first
    h = ctypes.cast(fake, vp)
    for nulls in ([0], [1], [2], [3], [4], [0, 1, 2, 3, 4]):
        a = [None if k in nulls else h for k in range(5)]
        assert L.sp_r1cs_check(a[0], a[1], a[2], a[3], a[4], ctypes.byref(v), ctypes.byref(f), None, sz(0)) == -1, nulls
    assert L.sp_r1cs_check(None, None, None, None, None, None, None, None, sz(0)) == -1
    assert v.value == 7 and f.value == 7     # nothing was written
    assert L.sp_strerror(-1).decode() != ""


def test_host_driver_exports_is_sat_and_python_binds_it():
    from spartan_amd import prover as P
    assert hasattr(P.H, "spz_instance_is_sat")
    assert callable(P.Instance.is_sat) and callable(P.Instance.check)
    hpp = open(os.path.join(ROOT, "spartan_amd", "host", "libspartan.hpp")).read()
    assert "struct SatReport" in hpp and hpp.count("bool is_sat(") == 2


def test_rust_seam_and_integration_name_the_entry_point():
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    seam = strip(open(os.path.join(ROOT, "rust_shim", "seams", "lib.rs")).read())
    tail = strip(open(os.path.join(ROOT, "rust_shim", "src", "gpu_tail.rs.in")).read())
    assert re.search(r"pub fn is_sat_gpu\(&self, vars: &VarsAssignment,\s*inputs: &InputsAssignment\) -> Result<\(bool, u64, Option<u64>\), R1CSError>", seam)
    assert "R1CSError::InvalidNumberOfInputs" in seam
    # the seam reaches the entry point: directly, or through a helper of the hand-written tail that it calls
    assert "sp_r1cs_check(" in seam or ("gpu::r1cs_check(" in seam and re.search(r"pub fn r1cs_check\(.*?sp_r1cs_check\(", tail, flags=re.S))
    # additive: the reference's own is_sat is not redefined, and the patch carries the seam
    assert not re.search(r"\bfn is_sat\(", seam)
    patch = open(os.path.join(ROOT, "rust_shim", "gpu_feature.patch")).read()
    assert "+  pub fn is_sat_gpu(" in patch and "sp_r1cs_check" in patch
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"Instance::is_sat.*sp_r1cs_check", integ)
