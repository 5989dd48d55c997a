"""CPU-side checks of the boundary of the byte parsers (sp_table_from_bytes and its three siblings, the spz_* exports of the host driver):
declared, exported and bound; null arguments are refused before a device is touched; the host parser spz_scalars_from_bytes, which needs no
device, reproduces the model of tests/assign_reference.py on every edge value and reports the refused entries."""
import ctypes, os, re
import pytest
from tests.helpers import ROOT, Q
from tests import assign_reference as ar

sz, vp = ctypes.c_size_t, ctypes.c_void_p
NEW = ["sp_table_from_bytes", "sp_table_from_bytes_dev", "sp_table_to_bytes", "sp_table_check_reduced"]
SPZ = ["spz_vars_assignment_from_bytes", "spz_vars_assignment_from_device_bytes", "spz_vars_assignment_len", "spz_vars_assignment_to_bytes",
       "spz_vars_assignment_check_reduced", "spz_scalars_from_bytes", "spz_scalars_to_bytes"]


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


def test_header_declares_the_entry_points_and_the_status():
    from spartan_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spartan_hip.h")).read(), flags=re.S)
    assert re.search(r"SP_ESCALAR\s*=\s*-5\b", hdr)
    want = {"sp_table_from_bytes": ["sp_ctx* ctx", "const uint8_t* bytes", "size_t n", "sp_table** out", "uint64_t* report"],
            "sp_table_from_bytes_dev": ["sp_ctx* ctx", "const uint8_t* dev_bytes", "size_t n", "sp_table** out", "uint64_t* report"],
            "sp_table_to_bytes": ["sp_ctx* ctx", "const sp_table* t", "size_t off", "size_t len", "uint8_t* out"],
            "sp_table_check_reduced": ["sp_ctx* ctx", "const sp_table* t", "size_t off", "size_t len", "uint64_t* report"]}
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want[name]
        assert hasattr(capi.lib, name) and name in capi.SYMBOLS
    assert capi.lib.sp_strerror(-5).decode() not in ("", "unknown")
    gpu_rs = open(os.path.join(ROOT, "rust_shim", "src", "gpu.rs")).read()
    assert "pub const SP_ESCALAR: i32 = -5;" in gpu_rs
    assert "pub fn sp_table_from_bytes(ctx: *mut sp_ctx, bytes: *const u8, n: usize, out: *mut *mut sp_table, report: *mut u64) -> i32;" in gpu_rs


def test_null_arguments_are_refused_without_a_device():
    """SP_EINVAL (-1), decided before any HIP call, and nothing is written"""
    from spartan_amd import capi
    L = capi.lib
    fake = ctypes.cast(ctypes.create_string_buffer(256), vp)   # never dereferenced: a null argument or n = 0 is found first
    data = bytes(64)
    out = vp(0x1234)
    rep = (ctypes.c_uint64 * 2)(7, 7)
    for f in (L.sp_table_from_bytes, L.sp_table_from_bytes_dev):
        assert f(None, data, sz(2), ctypes.byref(out), rep) == -1
        assert f(fake, None, sz(2), ctypes.byref(out), rep) == -1
        assert f(fake, data, sz(2), None, rep) == -1
        assert f(fake, data, sz(0), ctypes.byref(out), rep) == -1
    buf = (ctypes.c_uint8 * 64)(*([9] * 64))
    assert L.sp_table_to_bytes(None, fake, sz(0), sz(1), buf) == -1 and L.sp_table_to_bytes(fake, None, sz(0), sz(1), buf) == -1
    assert L.sp_table_check_reduced(None, fake, sz(0), sz(1), rep) == -1 and L.sp_table_check_reduced(fake, None, sz(0), sz(1), rep) == -1
    assert out.value == 0x1234 and list(rep) == [7, 7] and bytes(buf) == bytes([9] * 64)


def test_host_driver_exports_and_python_binds(P):
    for name in SPZ:
        assert hasattr(P.H, name), name
    for name in ("from_bytes", "from_tensor", "to_bytes", "check_reduced"):
        assert callable(getattr(P.VarsAssignment, name))
    assert callable(P.InputsAssignment.from_bytes) and callable(P.InputsAssignment.to_bytes)
    assert issubclass(P.InvalidScalar, P.SpartanHipError)
    assert "synchronise" in P.VarsAssignment.from_tensor.__doc__.lower()   # the caller's duty is written down


def _parse(P, data):
    n = len(data) // 32
    limbs = (ctypes.c_uint64 * (4 * max(n, 1)))(*([0xdead] * (4 * max(n, 1))))
    rep = (ctypes.c_uint64 * 2)(7, 7)
    rc = P.H.spz_scalars_from_bytes(bytes(data), sz(n), limbs, rep)
    return rc, list(limbs)[:4 * n], (int(rep[0]), int(rep[1])), P.H.spz_last_error().decode()


def test_host_parser_reproduces_the_model_on_every_edge_value(P):
    data = ar.enc(ar.EDGE_VALID)
    want, count, first = ar.from_bytes(data)
    rc, limbs, rep, _ = _parse(P, data)
    assert rc == 0 and limbs == want and rep == (0, ar.NONE)
    back = (ctypes.c_uint8 * len(data))()
    assert P.H.spz_scalars_to_bytes((ctypes.c_uint64 * len(limbs))(*limbs), sz(len(limbs) // 4), back) == 0
    assert bytes(back) == data == ar.to_bytes(want)
    for v in ar.EDGE_VALID:                                   # and one at a time
        rc, limbs, rep, _ = _parse(P, ar.enc([v]))
        assert rc == 0 and limbs == ar.from_bytes(ar.enc([v]))[0], hex(v)
    for v in ar.EDGE_INVALID:
        rc, limbs, rep, err = _parse(P, ar.enc([v]))
        assert rc == -1 and rep == (1, 0) and err.startswith("InvalidScalar"), hex(v)
        assert limbs == [0xdead] * 4                          # nothing written


def test_host_parser_reports_count_and_first(P):
    vals = ar.valid_values(33, 3)
    for pos in ([0], [16], [32], [5, 16], [0, 16, 32], list(range(33))):
        bad = list(vals)
        for k, p in enumerate(pos):
            bad[p] = ar.EDGE_INVALID[k % len(ar.EDGE_INVALID)]
        rc, _, rep, err = _parse(P, ar.enc(bad))
        assert rc == -1 and rep == (len(pos), pos[0]), pos
        assert err == "InvalidScalar: entry %d (%d of 33 entries are not canonical)" % (pos[0], len(pos))
        assert rep == ar.from_bytes(ar.enc(bad))[1:]
    rc, _, rep, err = _parse(P, ar.enc(vals))                 # the error of the last call does not linger
    assert rc == 0 and rep == (0, ar.NONE) and err == ""


def test_inputs_assignment_round_trip_and_error(P):
    vals = ar.valid_values(7, 11)
    limbs = P.InputsAssignment.from_bytes(ar.enc(vals))
    assert list(limbs) == ar.from_bytes(ar.enc(vals))[0]
    assert P.InputsAssignment.to_bytes(limbs) == ar.enc(vals)
    for data in (bytearray(ar.enc(vals)), memoryview(ar.enc(vals))):
        assert list(P.InputsAssignment.from_bytes(data)) == list(limbs)
    assert len(P.InputsAssignment.from_bytes(b"")) == 0
    bad = list(vals); bad[4] = Q; bad[6] = Q + 1
    with pytest.raises(P.InvalidScalar) as e:
        P.InputsAssignment.from_bytes(ar.enc(bad))
    assert (e.value.first, e.value.count) == (4, 2) and "InvalidScalar: entry 4" in str(e.value)
    with pytest.raises(P.SpartanHipError):
        P.InputsAssignment.from_bytes(bytes(33))


def test_rust_seam_and_documents_name_the_entry_points():
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    seam = strip(open(os.path.join(ROOT, "rust_shim", "seams", "lib.rs")).read())
    assert re.search(r"pub fn from_bytes_gpu\(assignment: &\[\[u8; 32\]\]\) -> Result<VarsAssignment, R1CSError>", seam)
    assert "sp_table_from_bytes(" in seam and "gpu::SP_ESCALAR" in seam and "R1CSError::InvalidScalar" in seam
    patch = open(os.path.join(ROOT, "rust_shim", "gpu_feature.patch")).read()
    assert "+  pub fn from_bytes_gpu(" in patch
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"Assignment::new.*sp_table_from_bytes", integ)
