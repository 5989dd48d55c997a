"""CPU-side checks of the boundary of the device build of R1CS matrices (sp_sparse_from_entries, sp_sparse_from_entries_dev,
sp_sparse_download_entries, the spz_* exports of the host driver): declared, exported and bound; the new status is known; every SP_EINVAL
condition is decided before a device is touched and leaves *out and the report as they were."""
import ctypes, os, re
import pytest
from tests.helpers import ROOT
from tests import sparse_build_reference as sb

sz, vp, u64 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint64
NEW = ["sp_sparse_from_entries", "sp_sparse_from_entries_dev", "sp_sparse_download_entries"]
SPZ = ["spz_instance_from_entries", "spz_instance_from_device_entries"]
GEOMETRY = ["uint64_t row_limit", "uint64_t col_limit", "uint64_t col_split", "uint64_t col_shift", "size_t pad_count", "uint64_t pad_col",
            "size_t num_rows", "size_t num_cols", "sp_sparse** out", "uint64_t* report"]


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


def test_header_declares_the_entry_points_and_the_status():
    from spartan_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spartan_hip.h")).read(), flags=re.S)
    assert re.search(r"SP_EINDEX\s*=\s*-6\b", hdr) and re.search(r"SP_ESCALAR\s*=\s*-5\b", hdr)
    want = {"sp_sparse_from_entries": ["sp_ctx* ctx", "const uint64_t* rows", "const uint64_t* cols", "const uint8_t* vals", "size_t nnz"] + GEOMETRY,
            "sp_sparse_from_entries_dev": ["sp_ctx* ctx", "const uint64_t* dev_rows", "const uint64_t* dev_cols", "const uint8_t* dev_vals", "size_t nnz"] + GEOMETRY,
            "sp_sparse_download_entries": ["sp_ctx* ctx", "const sp_sparse* m", "uint32_t* rows", "uint32_t* cols", "uint64_t* vals"]}
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want[name]
        assert hasattr(capi.lib, name) and name in capi.SYMBOLS
    msg = capi.lib.sp_strerror(-6).decode()
    assert msg not in ("", "unknown") and msg != capi.lib.sp_strerror(-5).decode() and capi.lib.sp_strerror(-7).decode() == "unknown"
    gpu_rs = open(os.path.join(ROOT, "rust_shim", "src", "gpu.rs")).read()
    assert "pub const SP_EINDEX: i32 = -6;" in gpu_rs and "pub fn sp_sparse_from_entries_dev(" in gpu_rs


def _call(f, ctx, rows, cols, vals, nnz, g, out, rep):
    return f(ctx, rows, cols, vals, sz(nnz), u64(g["row_limit"]), u64(g["col_limit"]), u64(g["col_split"]), u64(g["col_shift"]), sz(g["pad_count"]),
             u64(g["pad_col"]), sz(g["num_rows"]), sz(g["num_cols"]), out, rep)


def test_invalid_arguments_are_refused_without_a_device():
    """SP_EINVAL (-1), decided before any HIP call: neither *out nor the report is written. The conditions are those of the model."""
    from spartan_amd import capi
    L = capi.lib
    fake = ctypes.cast(ctypes.create_string_buffer(4096), vp)   # never dereferenced: the arguments are refused first
    rows, cols, vals = (u64 * 3)(0, 1, 2), (u64 * 3)(0, 1, 2), bytes(96)
    G = dict(row_limit=4, col_limit=7, col_split=5, col_shift=3, pad_count=0, pad_col=5, num_rows=4, num_cols=16)
    out = vp(0x1234)
    rep = (u64 * 4)(7, 7, 7, 7)
    o = ctypes.byref(out)
    for f in (L.sp_sparse_from_entries, L.sp_sparse_from_entries_dev):
        assert _call(f, None, rows, cols, vals, 3, G, o, rep) == -1
        assert _call(f, fake, None, cols, vals, 3, G, o, rep) == -1
        assert _call(f, fake, rows, None, vals, 3, G, o, rep) == -1
        assert _call(f, fake, rows, cols, None, 3, G, o, rep) == -1
        assert _call(f, fake, rows, cols, vals, 3, G, None, rep) == -1
        changes = [dict(num_rows=0), dict(num_cols=0), dict(row_limit=5), dict(col_limit=14), dict(col_shift=10), dict(col_shift=17),
                   dict(pad_count=2), dict(pad_count=1, pad_col=16), dict(num_rows=2**32), dict(num_cols=2**32), dict(pad_count=2**32 - 4),
                   dict(pad_count=2**64 - 1)]
        for change in changes:
            g = dict(G, **change)
            assert sb.invalid_arguments(3, g) or g["pad_count"] >= 2**32, change
            assert _call(f, fake, rows, cols, vals, 3, g, o, rep) == -1, change
        for nnz in (2**32 - 1, 2**32, 2**63):                     # nnz + pad_count >= 2^32 - 1
            assert sb.invalid_arguments(nnz, G) and _call(f, fake, rows, cols, vals, nnz, G, o, rep) == -1
        assert _call(f, None, None, None, None, 0, G, o, rep) == -1      # an empty matrix is legal, a null context is not
    assert out.value == 0x1234 and list(rep) == [7, 7, 7, 7]
    r32, buf = (ctypes.c_uint32 * 4)(9, 9, 9, 9), (u64 * 4)(9, 9, 9, 9)
    assert L.sp_sparse_download_entries(None, fake, r32, r32, buf) == -1 and L.sp_sparse_download_entries(fake, None, r32, r32, buf) == -1
    assert list(r32) == [9] * 4 and list(buf) == [9] * 4


def test_host_driver_exports_and_python_binds(P):
    for name in SPZ:
        assert hasattr(P.H, name), name
    assert callable(P.Instance.from_entries) and callable(P.Instance.from_tensors)
    assert issubclass(P.InvalidIndex, P.SpartanHipError) and issubclass(P.InvalidScalar, P.SpartanHipError)
    assert "synchronise" in P.Instance.from_tensors.__doc__.lower() and "unsigned" in P.Instance.from_tensors.__doc__.lower()
    with pytest.raises(P.SpartanHipError):                       # counts that do not add up are refused in Python, before any call
        P.Instance.from_entries(None, 2, 2, 0, [1, 1, 1], (u64 * 2)(), (u64 * 2)(), bytes(64))
    with pytest.raises(P.SpartanHipError):
        P.Instance.from_entries(None, 2, 2, 0, [1, 0, 0], (u64 * 1)(), (u64 * 1)(), bytes(33))


def test_rust_seam_and_documents_name_the_entry_points():
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    seam = strip(open(os.path.join(ROOT, "rust_shim", "seams", "lib.rs")).read())
    for name in NEW:
        assert name + "(" in seam, name
    assert "gpu::SP_EINDEX" in seam and "R1CSError::InvalidIndex" in seam and "R1CSError::InvalidScalar" in seam
    patch = open(os.path.join(ROOT, "rust_shim", "gpu_feature.patch")).read()
    assert "+  pub fn new_gpu(" in patch and "+pub const SP_EINDEX: i32 = -6;" in patch
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"Instance::new.*sp_sparse_from_entries", integ)
