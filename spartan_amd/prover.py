"""ctypes binding of the host-side prover driver (spartan_amd/host, libspartan_host.so), which mirrors libspartan's
SNARK/NIZK API on top of the HIP C ABI. No fallback: raises if either library is missing or no GPU is present."""
import ctypes, os
from .capi import SpartanHipError, LIB_PATH, sz, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_PATH = os.environ.get("SPARTAN_HOST_LIB") or os.path.join(_HERE, "lib", "libspartan_host.so")  # override: diagnostic builds (e.g. -DSPZ_HOSTPROF)
if not os.path.exists(HOST_PATH):
    raise SpartanHipError(f"{HOST_PATH} not built: run __graft_entry__.build()")
ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
H = ctypes.CDLL(HOST_PATH)
_i, _u64, _s, _ll = ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_longlong
_INST = [vp, sz, sz, sz, vp, vp, vp, vp]          # ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals
_BYTES = [vp, sz]                                 # out, cap of the size-then-fill idiom
_TAIL = [vp, vp]                                  # tape_seed, times10
_VERIFY = [vp, vp, vp, vp, sz, vp, sz]            # ctx, comm | inst, gens, proof, proof_len, inputs, n_inputs
_MANY = [vp, vp, vp, vp, vp, vp, sz, sz, _s, vp]  # ctx, comm | inst, gens, proofs, proof_lens, inputs, n_inputs, K, label, status_out
_SCRIPT = [_s, sz, vp, vp, vp, vp, vp]            # tlabel, nops, kinds, labels, datas, lens, out
# name -> (restype, argtypes) of every entry point include/spartan_host.h declares (tests/test_host_abi.py compares the two): every pointer is
# c_void_p (None, bytes, ctypes arrays, byref(), addresses and callbacks all pass), except the labels, which are c_char_p
SIGNATURES = {
    "spz_last_error": (_s, []),
    "spz_ctx_new": (vp, [_i]), "spz_ctx_free": (None, [vp]), "spz_ctx_raw": (vp, [vp]), "spz_ctx_set_option": (_i, [vp, _s, _s]),
    "spz_keccak_variant": (_s, []),
    "spz_ctx_set_commit_shard": (_i, [vp, _i, _i, vp, vp]), "spz_rccl_unique_id": (_i, [vp]),
    "spz_ctx_set_commit_shard_rccl": (_i, [vp, _i, _i, vp]), "spz_ctx_set_commit_shard_virtual": (_i, [vp, _i]),
    "spz_ctx_shard_stats": (None, [vp, _i, vp]),
    "spz_instance_new": (vp, _INST), "spz_instance_from_entries": (vp, _INST + [vp, vp, vp]),
    "spz_instance_from_device_entries": (vp, _INST + [vp, vp, vp]), "spz_instance_synthetic": (vp, [vp, sz, sz, sz, _u64, vp, vp]),
    "spz_instance_free": (None, [vp]), "spz_instance_digest": (sz, [vp] + _BYTES), "spz_instance_set_digest": (None, [vp, vp, sz]),
    "spz_instance_set_digest_header": (_i, [vp, _i]), "spz_instance_is_sat": (_i, [vp, vp, vp, sz, vp, sz, vp, vp, sz]),
    "spz_snark_gens_new": (vp, [vp, sz, sz, sz, sz]), "spz_nizk_gens_new": (vp, [vp, sz, sz, sz]),
    "spz_snark_verifier_gens_new": (vp, [vp, sz, sz, sz, sz]), "spz_nizk_verifier_gens_new": (vp, [vp, sz, sz, sz]),
    "spz_snark_gens_is_verifier_only": (_i, [vp]), "spz_nizk_gens_is_verifier_only": (_i, [vp]),
    "spz_snark_gens_resident_bytes": (sz, [vp]), "spz_nizk_gens_resident_bytes": (sz, [vp]),
    "spz_snark_gens_free": (None, [vp]), "spz_nizk_gens_free": (None, [vp]), "spz_snark_gens_stream": (sz, [vp, _i] + _BYTES),
    "spz_snark_gens_window_bits": (_i, [vp, _i]), "spz_snark_gens_windows": (_i, [vp, _i]), "spz_snark_gens_table_bytes": (sz, [vp, _i]),
    "spz_snark_gens_bincode": (sz, [vp] + _BYTES),
    "spz_snark_encode": (vp, [vp, vp, vp]), "spz_encode_free": (None, [vp]), "spz_commitment_bincode": (sz, [vp] + _BYTES),
    "spz_decommitment_bincode": (sz, [vp] + _BYTES), "spz_encode_comm": (sz, [vp, _i] + _BYTES),
    "spz_commitment_load": (vp, [vp, vp, sz]), "spz_commitment_encode": (vp, [vp, vp, vp]), "spz_commitment_serialize": (sz, [vp] + _BYTES),
    "spz_commitment_resident_bytes": (sz, [vp]), "spz_commitment_free": (None, [vp]),
    "spz_vars_assignment_new": (vp, [vp, vp, sz]), "spz_vars_assignment_free": (None, [vp]),
    "spz_vars_assignment_from_bytes": (vp, [vp, vp, sz, vp]), "spz_vars_assignment_from_device_bytes": (vp, [vp, vp, sz, vp]),
    "spz_vars_assignment_len": (sz, [vp]), "spz_vars_assignment_to_bytes": (_i, [vp, vp]), "spz_vars_assignment_check_reduced": (_i, [vp, vp]),
    "spz_scalars_from_bytes": (_i, [vp, sz, vp, vp]), "spz_scalars_to_bytes": (_i, [vp, sz, vp]),
    "spz_snark_prove": (vp, [vp, vp, vp, vp, vp, sz, vp, sz, _s] + _TAIL),
    "spz_snark_prove_resident": (vp, [vp, vp, vp, vp, vp, vp, sz, _s] + _TAIL),
    "spz_snark_prove_t": (vp, [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp] + _TAIL),
    "spz_nizk_prove": (vp, [vp, vp, vp, vp, sz, vp, sz, _s] + _TAIL),
    "spz_nizk_prove_resident": (vp, [vp, vp, vp, vp, vp, sz, _s] + _TAIL),
    "spz_nizk_prove_t": (vp, [vp, vp, vp, vp, vp, sz, vp, sz, vp] + _TAIL),
    "spz_proof_bytes": (sz, [vp] + _BYTES), "spz_proof_free": (None, [vp]), "spz_transcript_probe": (None, [vp, vp]),
    "spz_snark_verify": (_i, _VERIFY + [_s]), "spz_snark_verify_t": (_i, _VERIFY + [vp]),
    "spz_nizk_verify": (_i, _VERIFY + [_s]), "spz_nizk_verify_t": (_i, _VERIFY + [vp]),
    "spz_snark_verify_many": (_i, _MANY), "spz_nizk_verify_many": (_i, _MANY),
    # test hooks
    "spz_snark_reserialize": (_ll, [vp, sz] + _BYTES), "spz_nizk_parse_probe": (_ll, [vp, sz] + _BYTES),
    "spz_commitment_reserialize": (_ll, [vp, sz] + _BYTES), "spz_instance_shape_bincode": (sz, [vp] + _BYTES),
    "spz_zlib_level6": (sz, [vp, sz, _i] + _BYTES), "spz_zlib_probes": (sz, [vp, sz, ctypes.c_uint, _i] + _BYTES),
    "spz_deflate_matches_host": (None, [vp, sz, ctypes.c_uint, vp, vp, vp]),
    "spz_zlib_from_matches": (sz, [vp, sz, vp, vp, vp, ctypes.c_uint, _i] + _BYTES + [vp]),
    "spz_zlib_device": (sz, [vp, vp, sz, ctypes.c_uint, _i] + _BYTES + [vp]),
    "spz_instance_shape_bincode_device": (sz, [vp] + _BYTES), "spz_instance_digest_stats": (None, [vp, vp]),
    "spz_deflate_tokens_host": (sz, [vp, sz, ctypes.c_uint, vp, vp, vp]),
    "spz_zlib_from_tokens": (sz, [vp, sz, vp, sz, ctypes.c_uint, _i, sz] + _BYTES + [vp]),
    "spz_zlib_device_parse": (sz, [vp, vp, sz, ctypes.c_uint, _i, _i, sz, sz] + _BYTES + [vp, sz]),
    "spz_instance_digest_stats_all": (None, [vp, vp, sz]),
    "spz_deflate_blocks_host": (_ll, [vp, sz, sz, sz, vp, vp, sz, vp]),
    "spz_zlib_from_blocks": (sz, [vp, vp, sz, vp, vp, sz, ctypes.c_uint, _i] + _BYTES + [vp]),
    "spz_zlib_device_emit": (sz, [vp, vp, sz, ctypes.c_uint, _i, _i, sz, sz, sz] + _BYTES + [vp, sz]),
    "spz_keccak_run_variant": (_i, [_s, vp]), "spz_shake256": (None, [vp, sz, vp, sz]),
    "spz_merlin_script": (sz, _SCRIPT), "spz_merlin_state": (None, _SCRIPT), "spz_merlin_challenge_from_state": (None, [vp, _s, vp, sz]),
    "spz_tape_draws": (None, [vp, _s, sz, vp]), "spz_seed_scalar": (None, [_s, _u64, vp]),
    "spz_fq_invert_vartime": (None, [vp, vp]), "spz_unipoly_probe": (_i, [vp, sz, vp, vp, vp, vp]),
    "spz_cubic_coeffs_probe": (None, [vp, vp, vp]), "spz_cubic_tail_probe": (_i, [vp, sz, sz, vp, vp, vp]),
    "spz_eq_factor_probe": (_i, [vp, sz, sz, sz, vp, sz, vp, vp, vp, vp, vp]),
    "spz_rccl_allgather_probe": (ctypes.c_double, [vp, sz, _i]),
}
for _name, (_res, _args) in SIGNATURES.items():
    _f = getattr(H, _name)
    _f.restype, _f.argtypes = _res, _args
u64p = ctypes.POINTER(ctypes.c_uint64)
TIME_NAMES = ["polycommit", "prove_sc_phase_one", "prove_sc_phase_two", "polyeval", "R1CSProof::prove", "eval_sparse_polys",
              "commit_nondet_witness", "build_layered_network", "evalproof_layered_network", "total"]


def _failed(what):
    return f"{what} failed: {H.spz_last_error().decode()}"


def _chk(h, what):
    if not h:
        raise SpartanHipError(_failed(what))
    return vp(h)


def _fill(fn, *head, unit=1):
    """the size-then-fill idiom of spartan_host.h: ask for the size (in units of `unit` bytes), then for the bytes"""
    n = unit * fn(*head, None, 0)
    b = (ctypes.c_uint8 * n)()
    fn(*head, b, n)
    return bytes(b)


def _limbs_or_handle(vars_):
    """(assignment, vars, nvars) as the entries that take either take them: a VarsAssignment, or Montgomery limbs read in place"""
    return (vars_.h, None, 0) if isinstance(vars_, VarsAssignment) else (None, vars_, len(vars_) // 4)


def _n_inputs(inst, inputs):
    return inst.num_inputs if inputs is inst.inputs else len(inputs) // 4   # the instance's own buffer holds one element when num_inputs is 0


class Ctx:
    def __init__(self, device=0):
        self.h = _chk(H.spz_ctx_new(device), "spz_ctx_new")

    def raw(self):
        """the underlying sp_ctx* (for profiling calls through spartan_amd.capi.lib)"""
        return vp(H.spz_ctx_raw(self.h))

    def set_option(self, key, value):
        """a library option of this context (sp_ctx_set_option; table: spartan_amd/csrc/options.hpp). Tier-1 (A/B / test) options need
        set_option("testing.unlock", 1) first."""
        if H.spz_ctx_set_option(self.h, key.encode(), str(int(value)).encode()) != 0:
            raise SpartanHipError(f"set_option({key}, {value}) refused")

    def set_commit_shard(self, dist, device="cpu"):
        """row-shard every DensePolynomial::commit over the ranks of `dist`, the bytes moved by torch.distributed
        (spartan_amd/shard.py; gloo in the CPU tests); None clears it. All ranks must then run identical prove() calls in lock-step."""
        from . import shard
        if dist is None or dist.get_world_size() == 1:
            H.spz_ctx_set_commit_shard(self.h, 0, 1, None, None); self._gather = None
            return
        self._gather = shard.make_gather_callback(dist, device)
        if H.spz_ctx_set_commit_shard(self.h, dist.get_rank(), dist.get_world_size(), self._gather, None) != 0:
            raise SpartanHipError(f"set_commit_shard: {H.spz_last_error().decode()}")

    def set_commit_shard_rccl(self, rank, world, unique_id):
        """the same with RCCL inside the library: `unique_id` = the 128 bytes rank 0 got from rccl_unique_id(), handed to
        every rank by the caller (bench.py: one torch.distributed broadcast); ncclAllGather on device buffers per commit"""
        if H.spz_ctx_set_commit_shard_rccl(self.h, rank, world, unique_id) != 0:
            raise SpartanHipError(f"set_commit_shard_rccl: {H.spz_last_error().decode()}")

    def set_commit_shard_virtual(self, nshards):
        """nshards row shards on this one GPU (sub-contexts with their own streams, in-process gather); <= 1 clears it"""
        if H.spz_ctx_set_commit_shard_virtual(self.h, nshards) != 0:
            raise SpartanHipError(f"set_commit_shard_virtual: {H.spz_last_error().decode()}")

    def shard_stats(self, reset=False):
        out = (ctypes.c_uint64 * 2)()
        H.spz_ctx_shard_stats(self.h, 1 if reset else 0, out)
        return {"gathers": int(out[0]), "bytes": int(out[1])}

    def close(self):
        if self.h:
            H.spz_ctx_free(self.h); self.h = None


class Instance:
    def __init__(self, h, num_cons, num_vars, num_inputs, vars_=None, inputs=None):
        self.h, self.num_cons, self.num_vars, self.num_inputs, self.vars, self.inputs = h, num_cons, num_vars, num_inputs, vars_, inputs

    @staticmethod
    def new(ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals):
        """Instance::new (lib.rs:121): entries of A, B, C back to back; vals = 32 canonical little-endian bytes each."""
        h = _chk(H.spz_instance_new(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs), (sz * 3)(*nnz), rows, cols, vals), "Instance::new")
        return Instance(h, num_cons, num_vars, num_inputs)

    @staticmethod
    def from_entries(ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals):
        """Instance::new (lib.rs:121) built on the device: the arguments of Instance.new (entries of A, B, C back to back, nnz = their three
        counts, rows and cols as ctypes uint64 arrays), `vals` any buffer of 32 n bytes. Only the indices and the bytes cross PCIe: the index
        test, the comparison with q, the Montgomery form, the column shift, the pad entries and the row- and column-sorted copies are made in
        HBM (sp_sparse_from_entries), and the instance keeps no host copy of its entries. Raises InvalidIndex or InvalidScalar for the first
        matrix that fails and, within it, the lowest failing entry, as the reference's loops return."""
        what = "Instance::from_entries"
        buf, n = _byte_buffer(vals, what)
        nnz = [int(x) for x in nnz]
        if len(nnz) != 3 or sum(nnz) != n or len(rows) < n or len(cols) < n:
            raise SpartanHipError(f"{what}: {nnz} entries announced, {len(rows)} rows, {len(cols)} columns and {n} values given")
        st, mat, rep = ctypes.c_int32(), ctypes.c_int(), (ctypes.c_uint64 * 4)()
        h = H.spz_instance_from_entries(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs), (sz * 3)(*nnz), rows, cols, buf, ctypes.byref(st),
                                        ctypes.byref(mat), rep)
        _entries_result(h, st, mat, rep, what)
        return Instance(vp(h), num_cons, num_vars, num_inputs)

    @staticmethod
    def from_tensors(ctx, num_cons, num_vars, num_inputs, A, B, C):
        """The same from entry lists already on the context's GPU: each of A, B, C is (rows, cols, vals) with rows and cols torch.int64 tensors
        of n elements, READ AS UNSIGNED (a negative value is an InvalidIndex), and vals a torch.uint8 tensor of 32 n elements; all contiguous,
        views at any offset allowed, n = 0 allowed. Nothing visits host memory. THE CALLER SYNCHRONISES the stream that wrote the tensors
        before the call (torch.cuda.synchronize(), or a synchronize of that stream): the library copies on its own stream, which is not
        ordered against torch's. Raises InvalidIndex / InvalidScalar like from_entries."""
        import torch
        from .capi import lib
        what = "Instance::from_tensors"
        dev = int(lib.sp_ctx_device(ctx.raw()))
        nnz, ptrs = [], ([], [], [])
        for name, m in zip("ABC", (A, B, C)):
            if len(m) != 3:
                raise SpartanHipError(f"{what}: matrix {name} is not (rows, cols, vals)")
            r, c, v = m
            for t, dt in ((r, torch.int64), (c, torch.int64), (v, torch.uint8)):
                if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or t.device.index != dev or not t.is_contiguous():
                    raise SpartanHipError(f"{what}: matrix {name} needs contiguous torch.int64 rows and cols and torch.uint8 vals on device {dev}")
            n = r.numel()
            if c.numel() != n or v.numel() != 32 * n:
                raise SpartanHipError(f"{what}: matrix {name} has {n} rows, {c.numel()} cols and {v.numel()} value bytes")
            nnz.append(n)
            for lst, t in zip(ptrs, (r, c, v)):
                lst.append(t.data_ptr() if n else None)
        st, mat, rep = ctypes.c_int32(), ctypes.c_int(), (ctypes.c_uint64 * 4)()
        h = H.spz_instance_from_device_entries(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs), (sz * 3)(*nnz), (vp * 3)(*ptrs[0]), (vp * 3)(*ptrs[1]),
                                               (vp * 3)(*ptrs[2]), ctypes.byref(st), ctypes.byref(mat), rep)
        _entries_result(h, st, mat, rep, what)
        return Instance(vp(h), num_cons, num_vars, num_inputs)

    @staticmethod
    def produce_synthetic_r1cs(ctx, num_cons, num_vars, num_inputs, seed=0):
        v = (ctypes.c_uint64 * (4 * num_vars))(); i = (ctypes.c_uint64 * (4 * max(num_inputs, 1)))()
        h = _chk(H.spz_instance_synthetic(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs), ctypes.c_uint64(seed), v, i), "produce_synthetic_r1cs")
        return Instance(h, num_cons, num_vars, num_inputs, v, i)

    def set_digest(self, d):
        H.spz_instance_set_digest(self.h, d, sz(len(d)))

    def digest(self):
        """R1CSShapeDigest (src/r1cs.rs:154-158): the bytes set with set_digest, else computed by the host library (zlib level 6 of bincode(shape))"""
        d = _fill(H.spz_instance_digest, self.h)
        if not d:   # a zlib stream is never empty: the computation failed
            raise SpartanHipError(_failed("Instance::digest"))
        return d

    def digest_stats(self):
        """figures of the last digest computation (see zlib_device); the host path (option digest.device = 0) fills ms_total only"""
        st = (ctypes.c_double * len(DEFLATE_STATS))()
        H.spz_instance_digest_stats_all(self.h, st, sz(len(DEFLATE_STATS)))
        return dict(zip(DEFLATE_STATS, st))

    def shape_bincode_device(self):
        """test hook: bincode(R1CSShape) with the matrices serialised on the device (sp_sparse_bincode)"""
        b = _fill(H.spz_instance_shape_bincode_device, self.h)
        if not b:
            raise SpartanHipError(_failed("Instance::shape_bincode_device"))
        return b

    def set_digest_header(self, old_header):
        """zlib header variant of the computed digest: False = 0x78 0x9C (miniz >= 2.2, miniz_oxide >= 0.4), True = 0x78 0x01"""
        if H.spz_instance_set_digest_header(self.h, 1 if old_header else 0) != 0:
            raise SpartanHipError("set_digest_header: " + H.spz_last_error().decode())

    def check(self, vars_, inputs, max_rows=16):
        """Instance::is_sat (lib.rs:230-259) on the device, with a report: .violated = the number of constraints the assignment fails,
        .first_row = the smallest of them (None when satisfied), .rows = the lowest max_rows of them, ascending. vars_: Montgomery limbs
        (a ctypes uint64 array; fewer than num_vars are zero-padded) or a VarsAssignment. Raises SpartanHipError("InvalidNumberOfInputs")
        where the reference returns that R1CSError: too many variables, or a number of inputs other than num_inputs."""
        rep = (ctypes.c_uint64 * 2)()
        rows = (ctypes.c_uint64 * max(max_rows, 1))()
        rc = H.spz_instance_is_sat(self.h, *_limbs_or_handle(vars_), inputs, _n_inputs(self, inputs), rep, rows if max_rows > 0 else None, max_rows)
        if rc < 0:
            raise SpartanHipError(_failed("Instance::is_sat"))
        violated = int(rep[0])
        return SatReport(violated, int(rep[1]) if violated else None, [int(r) for r in rows[:min(violated, max_rows)]])

    def is_sat(self, vars_, inputs):
        return self.check(vars_, inputs, max_rows=0).violated == 0

    def free(self):
        if self.h:
            H.spz_instance_free(self.h); self.h = None


class SatReport:
    """what Instance.check found (bool(report): the assignment satisfies the instance)"""
    def __init__(self, violated, first_row, rows):
        self.violated, self.first_row, self.rows = violated, first_row, rows

    def __bool__(self):
        return self.violated == 0

    def __repr__(self):
        return f"SatReport(violated={self.violated}, first_row={self.first_row}, rows={self.rows})"


class SNARKGens:
    def __init__(self, ctx, num_cons, num_vars, num_inputs, num_nz_entries):
        self.h = _chk(H.spz_snark_gens_new(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs), sz(num_nz_entries)), "SNARKGens::new")

    @classmethod
    def verifier_only(cls, ctx, num_cons, num_vars, num_inputs, num_nz_entries):
        """the generators of a process that only verifies: the same streams (stream(which) gives the same bytes) held as resident point
        sets of 64 KiB a point, without the prover's fixed-base window tables. SNARK.verify / verify_status / verify_t / verify_many take
        them; SNARK.encode, SNARK.prove* and the window-table accessors raise SpartanHipError."""
        g = cls.__new__(cls)
        g.h = _chk(H.spz_snark_verifier_gens_new(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs), sz(num_nz_entries)), "SNARKGens::verifier_only")
        return g

    @property
    def is_verifier_only(self):
        return bool(H.spz_snark_gens_is_verifier_only(self.h))

    def resident_bytes(self):
        """HBM held by the tables of the two generator streams (verifier-only: 65536 bytes a point)"""
        return int(H.spz_snark_gens_resident_bytes(self.h))

    def stream(self, which):
        return _fill(H.spz_snark_gens_stream, self.h, which)

    def window_bits(self, which):
        """signed window width of the fixed-base tables of generator stream `which` (0: gens_r1cs_sat, 1: gens_r1cs_eval)"""
        return self._tables(H.spz_snark_gens_window_bits(self.h, which), "window_bits")

    def _tables(self, value, what):
        if int(value) <= 0 and self.is_verifier_only:
            raise SpartanHipError(_failed(f"SNARKGens::{what}"))
        return int(value)

    def windows(self, which):
        """windows per scalar (= mixed additions per committed scalar) of the tables of generator stream `which`"""
        return self._tables(H.spz_snark_gens_windows(self.h, which), "windows")

    def table_bytes(self, which):
        """HBM held by the window tables of generator stream `which`"""
        return self._tables(H.spz_snark_gens_table_bytes(self.h, which), "table_bytes")

    def serialize(self):
        return _fill(H.spz_snark_gens_bincode, self.h)

    def free(self):
        if self.h:
            H.spz_snark_gens_free(self.h); self.h = None


class NIZKGens:
    def __init__(self, ctx, num_cons, num_vars, num_inputs):
        self.h = _chk(H.spz_nizk_gens_new(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs)), "NIZKGens::new")

    @classmethod
    def verifier_only(cls, ctx, num_cons, num_vars, num_inputs):
        """the generators of a process that only verifies (see SNARKGens.verifier_only): for NIZK.verify / verify_status / verify_t /
        verify_many; NIZK.prove* raise SpartanHipError"""
        g = cls.__new__(cls)
        g.h = _chk(H.spz_nizk_verifier_gens_new(ctx.h, sz(num_cons), sz(num_vars), sz(num_inputs)), "NIZKGens::verifier_only")
        return g

    @property
    def is_verifier_only(self):
        return bool(H.spz_nizk_gens_is_verifier_only(self.h))

    def resident_bytes(self):
        """HBM held by the tables of the generator stream (verifier-only: 65536 bytes a point)"""
        return int(H.spz_nizk_gens_resident_bytes(self.h))

    def free(self):
        if self.h:
            H.spz_nizk_gens_free(self.h); self.h = None


def rccl_unique_id():
    """ncclGetUniqueId through the library (rank 0 calls it; the 128 bytes go to every rank)"""
    out = (ctypes.c_uint8 * 128)()
    if H.spz_rccl_unique_id(out) != 0:
        raise SpartanHipError(f"rccl_unique_id: {H.spz_last_error().decode()}")
    return bytes(out)


def keccak_variant():
    """which form of Keccak-f[1600] the host driver picked for this CPU (keccak.cc): plain | bmi2 | avx512"""
    return H.spz_keccak_variant().decode()


DEFLATE_STATS = ("lookups", "fallbacks", "segments", "ms_links", "ms_search_a", "ms_search_b", "ms_download", "ms_parse", "ms_wait", "ms_stream",
                 "ms_total", "device", "parse", "tokens", "device_fallbacks", "ms_reach", "ms_emit",
                 "emit", "tokens_coded", "blocks", "stored_blocks", "static_blocks", "ms_blocks", "ms_bits", "ms_tables", "ms_bytes")


def zlib_device(ctx, data, probes=128, old_header=False, parse=0, tile=0, group=0, chunk=0):
    """(zlib stream of `data` as miniz writes it at this tdefl probe count, stats): the device-assisted deflate the instance digest runs over
    bincode(shape) — match search on the GPU in segments of the option digest.segment, parser and Huffman coding on the calling thread; with
    parse = 1 the lazy parse on the GPU too (tiles of `tile` positions, groups of `group` tiles; 0: the defaults) and only the token coder on
    the calling thread; parse = None: as the option digest.device says (2 = the device parse), which is what Instance.digest() follows.
    stats: lookups and those neither match table answered, segments, device ms of links / search A / search B / downloads, host ms of parse /
    wait / stream / total; parse = 1.0 when the device parsed, its tokens, the look-ups it searched on the spot, device ms of the reachability
    kernels and of the token kernel with its compaction (ms_parse is then the token coder alone). parse = 2 (digest.device = 3): the coder's
    block boundaries, histograms, bit emission (`chunk` tokens a workgroup; 0: the default), stored-block copies and Adler-32 on the GPU as
    well, the calling thread builds each block's Huffman tables and bit offsets from its histogram: emit = 1.0, tokens stays 0 (none comes
    down) and tokens_coded counts them, blocks / stored_blocks / static_blocks, device ms of the block stage and of the bit emission, host ms
    of the table building (within ms_parse) and of the download of the compressed bytes."""
    data = bytes(data)
    cap = 2 * len(data) + 1024
    out = (ctypes.c_uint8 * cap)(); st = (ctypes.c_double * len(DEFLATE_STATS))()
    n = H.spz_zlib_device_emit(ctx.h, data, sz(len(data)), ctypes.c_uint(probes), 1 if old_header else 0, -1 if parse is None else int(parse),
                               sz(tile), sz(group), sz(chunk), out, sz(cap), st, sz(len(DEFLATE_STATS)))
    if n == 0:
        raise SpartanHipError(_failed("zlib_device"))
    return bytes(out[:n]), dict(zip(DEFLATE_STATS, st))


def deflate_tokens(ctx, data, probes=128, tile=0, group=0):
    """test hook: (tokens of tdefl's lazy parse of `data` as the device produces them (sp_deflate_tokens), segments entered with a held match,
    look-ups the device searched on the spot). A token is one 32-bit word, see include/spartan_hip.h."""
    from .capi import lib
    data = bytes(data)
    n = len(data)
    tok = (ctypes.c_uint32 * max(1, n))(); ntok = ctypes.c_size_t(0); info = (ctypes.c_uint64 * 2)()
    buf = (ctypes.c_uint8 * max(1, n)).from_buffer_copy(data) if n else (ctypes.c_uint8 * 1)()
    rc = lib.sp_deflate_tokens(ctx.raw(), buf, sz(n), ctypes.c_int(0), ctypes.c_uint32(probes), sz(tile), sz(group), tok, ctypes.byref(ntok), info)
    if rc != 0:
        raise SpartanHipError("sp_deflate_tokens failed: %d" % rc)
    return tok, ntok.value, info[0], info[1]


def deflate_blocks(ctx, data, probes=128, tile=0, group=0):
    """test hook: (block records, histograms, their number) of `data` as the device finds them (sp_deflate_blocks): 6 64-bit words and 320
    16-bit counters a block, laid out as spz_deflate_blocks_host's (include/spartan_host.h)."""
    from .capi import lib
    data = bytes(data)
    n = len(data)
    cap = n // 11306 + 4     # a block that is not the last holds more than 11306 tokens (include/spartan_hip.h)
    rec = (ctypes.c_uint64 * (6 * cap))(); hist = (ctypes.c_uint16 * (320 * cap))(); nb = ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * max(1, n)).from_buffer_copy(data) if n else (ctypes.c_uint8 * 1)()
    rc = lib.sp_deflate_blocks(ctx.raw(), buf, sz(n), ctypes.c_int(0), ctypes.c_uint32(probes), sz(tile), sz(group), rec, hist, sz(cap), ctypes.byref(nb))
    if rc != 0:
        raise SpartanHipError("sp_deflate_blocks failed: %d" % rc)
    return rec, hist, nb.value


def seed_scalar(domain, seed):
    """TEST/BENCH ONLY: the reproducible 64-bit-seed -> scalar map behind the RandomTape seeds of tests/ and bench.py. A real
    proof passes tape_seed=None (the tape is then seeded from OS entropy, like RandomTape::new, random.rs:13-15): a known or
    reused seed fixes every blind of the proof and gives up zero-knowledge."""
    out = (ctypes.c_uint64 * 4)()
    H.spz_seed_scalar(domain, seed, out)
    return out


def _prove(what, entry, head, inst, vars_, inputs, transcript, tape_seed, times=None):
    """one proof. entry = (the entry for host limbs, the one for a VarsAssignment) of a proof on a fresh transcript, `transcript` its label; or
    the one *_prove_t entry, which takes either assignment, `transcript` the caller's state. head = the handles in front of the assignment."""
    tm = (ctypes.c_double * 10)()
    if not isinstance(entry, tuple):
        vars_args = _limbs_or_handle(vars_)
    elif isinstance(vars_, VarsAssignment):
        entry, vars_args = entry[1], (vars_.h,)
    else:
        entry, vars_args = entry[0], (vars_, len(vars_) // 4)
    p = _chk(entry(*head, *vars_args, inputs, inst.num_inputs, transcript, tape_seed, tm), what)
    if times is not None:
        times.update(dict(zip(TIME_NAMES, list(tm))))
    b = _fill(H.spz_proof_bytes, p)
    H.spz_proof_free(p)
    return b


def _verify_many(who, fn, ctx, subject, proofs, inputs, gens, transcript_label, count):
    """the body of SNARK.verify_many and NIZK.verify_many: subject = the Commitment / the Instance, count(buffer) = its number of inputs"""
    K = len(proofs)
    per = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs] * K
    if len(per) != K:
        raise SpartanHipError(f"{who}::verify_many failed: one inputs buffer per proof")
    sizes = {count(x) for x in per}
    if len(sizes) > 1:
        raise SpartanHipError(f"{who}::verify_many failed: InvalidNumberOfInputs")
    keep = [ctypes.create_string_buffer(bytes(p), max(len(p), 1)) for p in proofs]
    pa = (vp * K)(*[ctypes.cast(b, vp) for b in keep])
    la = (sz * K)(*[len(p) for p in proofs])
    ia = (vp * K)(*[ctypes.cast(x, vp) for x in per])
    st = (ctypes.c_int * K)()
    if fn(ctx.h, subject.h, gens.h, pa, la, ia, sizes.pop() if K else 0, K, transcript_label, st) != 0:
        raise SpartanHipError(_failed(f"{who}::verify_many"))
    return [int(x) for x in st]


def _verdict(rc, what):
    if rc < -1:
        raise SpartanHipError(_failed(what))
    return int(rc)


class SNARK:
    @staticmethod
    def encode(ctx, inst, gens):
        return Encoded(_chk(H.spz_snark_encode(ctx.h, inst.h, gens.h), "SNARK::encode"))

    @staticmethod
    def prove(ctx, inst, enc, vars_, inputs, gens, transcript_label, tape_seed, times=None):
        """vars_: the assignment as Montgomery limbs (a ctypes uint64 array, read in place) or a VarsAssignment (already in HBM)"""
        return _prove("SNARK::prove", (H.spz_snark_prove, H.spz_snark_prove_resident), (ctx.h, inst.h, gens.h, enc.h), inst, vars_, inputs,
                      transcript_label, tape_seed, times)

    @staticmethod
    def prove_t(ctx, inst, enc, vars_, inputs, gens, transcript_state, tape_seed):
        """SNARK::prove on a caller-owned transcript (lib.rs:339-347): `transcript_state` is a 203-byte ctypes array holding the
        merlin transcript (Strobe128 state, pos, pos_begin, cur_flags); it is continued by the proof and left in the state the
        proof ends in. Returns the proof bytes."""
        return _prove("SNARK::prove", H.spz_snark_prove_t, (ctx.h, inst.h, gens.h, enc.h), inst, vars_, inputs, transcript_state, tape_seed)

    @staticmethod
    def verify_status(ctx, comm, proof_bytes, inputs, gens, transcript_label):
        """SNARK::verify (lib.rs:423-466) of untrusted proof bytes against a Commitment, on the device: 1 accept, 0 reject, -1 malformed bytes.
        `inputs`: Montgomery limbs (a ctypes uint64 array). Raises SpartanHipError("InvalidNumberOfInputs") when their number is not the
        commitment's num_inputs, as NIZK.verify_status does."""
        return _verdict(H.spz_snark_verify(ctx.h, comm.h, gens.h, bytes(proof_bytes), len(proof_bytes), inputs, len(inputs) // 4, transcript_label),
                        "SNARK::verify")

    @staticmethod
    def verify(ctx, comm, proof_bytes, inputs, gens, transcript_label):
        """True when the proof is accepted; False for a rejected AND for a malformed proof (verify_status tells them apart)"""
        return SNARK.verify_status(ctx, comm, proof_bytes, inputs, gens, transcript_label) == 1

    @staticmethod
    def verify_many(ctx, comm, proofs, inputs, gens, transcript_label):
        """SNARK::verify of many untrusted proofs of ONE circuit in lock step on the device (spz_snark_verify_many): the list of
        verify_status's verdicts, 1 accept, 0 reject, -1 malformed bytes, one per proof — every proof is verified as verify_status verifies it,
        but the K verifications share their device round trips (8 for up to 64 proofs). `inputs`: one buffer of Montgomery limbs (a ctypes
        uint64 array) shared by all proofs, or a list with one buffer per proof. Raises SpartanHipError("InvalidNumberOfInputs") when a buffer's
        size is not the commitment's num_inputs, and for a device failure; no verdicts then."""
        return _verify_many("SNARK", H.spz_snark_verify_many, ctx, comm, proofs, inputs, gens, transcript_label, lambda x: len(x) // 4)

    @staticmethod
    def verify_t(ctx, comm, proof_bytes, inputs, gens, transcript_state):
        """SNARK::verify on a caller-owned transcript: the 203-byte state (see prove_t) is continued by the verification and left in the state
        it ends in — after an accepted proof, the state SNARK.prove_t left on the prover's side. Returns the status of verify_status."""
        return _verdict(H.spz_snark_verify_t(ctx.h, comm.h, gens.h, bytes(proof_bytes), len(proof_bytes), inputs, len(inputs) // 4, transcript_state),
                        "SNARK::verify")


class Commitment:
    """the verifier's handle of a circuit: a ComputationCommitment parsed from its (untrusted) bincode bytes (load), or computed from the
    instance itself (encode)"""
    def __init__(self, h):
        self.h = h

    @staticmethod
    def load(ctx, comm_bytes):
        """raises SpartanHipError for bytes that are not one commitment (ComputationCommitment::deserialize, libspartan.hpp)"""
        return Commitment(_chk(H.spz_commitment_load(ctx.h, bytes(comm_bytes), len(comm_bytes)), "Commitment.load"))

    @staticmethod
    def encode(ctx, inst, gens):
        """the commitment half of SNARK::encode (lib.rs:325-336: public preprocessing) run by the verifier, under either kind of SNARKGens:
        with SNARKGens.verifier_only the two commitments are computed over the resident point sets and no window table is built. The dense
        representation is dropped; no decommitment is kept. serialize() gives the bytes SNARK.encode(...).serialize_commitment() gives."""
        return Commitment(_chk(H.spz_commitment_encode(ctx.h, inst.h, gens.h), "Commitment.encode"))

    def serialize(self):
        """bincode(ComputationCommitment) of the handle, however it was made"""
        return _fill(H.spz_commitment_serialize, self.h)

    def resident_bytes(self):
        """HBM held by the two share vectors as resident point sets: 65536 bytes a share"""
        return int(H.spz_commitment_resident_bytes(self.h))

    def free(self):
        if self.h:
            H.spz_commitment_free(self.h); self.h = None


class NIZK:
    @staticmethod
    def prove_t(ctx, inst, vars_, inputs, gens, transcript_state, tape_seed):
        """NIZK::prove on a caller-owned transcript (lib.rs:501-509); see SNARK.prove_t"""
        return _prove("NIZK::prove", H.spz_nizk_prove_t, (ctx.h, inst.h, gens.h), inst, vars_, inputs, transcript_state, tape_seed)

    @staticmethod
    def verify_status(ctx, inst, proof_bytes, inputs, gens, transcript_label):
        """NIZK::verify (lib.rs:549-587) of untrusted proof bytes on the device: 1 accept, 0 reject, -1 malformed bytes. `inputs`: Montgomery limbs
        (a ctypes uint64 array) or the instance's own. Raises SpartanHipError("InvalidNumberOfInputs") for a wrong number of inputs, as
        Instance.is_sat does."""
        return _verdict(H.spz_nizk_verify(ctx.h, inst.h, gens.h, bytes(proof_bytes), len(proof_bytes), inputs, _n_inputs(inst, inputs), transcript_label),
                        "NIZK::verify")

    @staticmethod
    def verify(ctx, inst, proof_bytes, inputs, gens, transcript_label):
        """True when the proof is accepted; False for a rejected AND for a malformed proof (verify_status tells them apart)"""
        return NIZK.verify_status(ctx, inst, proof_bytes, inputs, gens, transcript_label) == 1

    @staticmethod
    def verify_many(ctx, inst, proofs, inputs, gens, transcript_label):
        """NIZK::verify of many untrusted proofs of ONE instance in lock step on the device (spz_nizk_verify_many): the list of verify_status's
        verdicts, 1 accept, 0 reject, -1 malformed bytes, one per proof — every proof is verified as verify_status verifies it, but the K
        verifications share their device round trips, and the instance is evaluated at the K proofs' points in one pass over its matrices.
        `inputs`: one buffer of Montgomery limbs (a ctypes uint64 array, or the instance's own) shared by all proofs, or a list with one buffer
        per proof. Raises SpartanHipError("InvalidNumberOfInputs") when a buffer's size is not the instance's num_inputs, and for a device
        failure; no verdicts then."""
        return _verify_many("NIZK", H.spz_nizk_verify_many, ctx, inst, proofs, inputs, gens, transcript_label, lambda x: _n_inputs(inst, x))

    @staticmethod
    def verify_t(ctx, inst, proof_bytes, inputs, gens, transcript_state):
        """NIZK::verify on a caller-owned transcript: the 203-byte state (see SNARK.prove_t) is continued by the verification and left in the
        state it ends in — after an accepted proof, the state NIZK.prove_t left on the prover's side. Returns the status of verify_status."""
        return _verdict(H.spz_nizk_verify_t(ctx.h, inst.h, gens.h, bytes(proof_bytes), len(proof_bytes), inputs, _n_inputs(inst, inputs), transcript_state),
                        "NIZK::verify")

    @staticmethod
    def prove(ctx, inst, vars_, inputs, gens, transcript_label, tape_seed, times=None):
        return _prove("NIZK::prove", (H.spz_nizk_prove, H.spz_nizk_prove_resident), (ctx.h, inst.h, gens.h), inst, vars_, inputs, transcript_label,
                      tape_seed, times)


class InvalidScalar(SpartanHipError):
    """R1CSError::InvalidScalar (lib.rs:75-79, 184-186): a 32-byte string of an assignment or of a matrix entry is not a canonical scalar (its
    value is >= q). .first = the lowest index of such an entry, .count = how many there are; from Instance.from_entries / from_tensors also
    .matrix = 0, 1, 2 for A, B, C (None for an assignment), and the count is taken among the entries whose index is good."""
    def __init__(self, what, first, count, matrix=None):
        super().__init__(_failed(what))
        self.first, self.count, self.matrix = first, count, matrix


class InvalidIndex(SpartanHipError):
    """R1CSError::InvalidIndex (lib.rs:164-172) from Instance.from_entries / from_tensors: an entry names a row >= num_cons or a column >=
    num_vars + 1 + num_inputs. .matrix = 0, 1, 2 for A, B, C, .first = the lowest such entry of that matrix, .count = how many it has."""
    def __init__(self, what, first, count, matrix):
        super().__init__(_failed(what))
        self.first, self.count, self.matrix = first, count, matrix


def _entries_result(h, st, mat, rep, what):
    if h:
        return
    if st.value == -6:    # SP_EINDEX
        raise InvalidIndex(what, int(rep[1]), int(rep[0]), int(mat.value))
    if st.value == -5:    # SP_ESCALAR
        raise InvalidScalar(what, int(rep[3]), int(rep[2]), int(mat.value))
    raise SpartanHipError(_failed(what))


def _byte_buffer(data, what):
    """(object ctypes passes as a pointer, number of scalars) for any contiguous buffer of 32 n bytes; bytes and writable buffers are read in place"""
    if not isinstance(data, bytes):
        mv = memoryview(data)
        if not mv.c_contiguous:
            raise SpartanHipError(f"{what}: the buffer is not contiguous")
        mv = mv.cast("B")
        data = bytes(mv) if mv.readonly else (ctypes.c_uint8 * len(mv)).from_buffer(mv)
    if len(data) % 32:
        raise SpartanHipError(f"{what}: {len(data)} bytes are not a whole number of 32-byte scalars")
    return data, len(data) // 32


def _scalar_result(ok, rep, what):
    if not ok:
        if H.spz_last_error().startswith(b"InvalidScalar"):
            raise InvalidScalar(what, int(rep[1]), int(rep[0]))
        raise SpartanHipError(_failed(what))


class VarsAssignment:
    """VarsAssignment::new (lib.rs:56-105) with the scalars uploaded once: proofs over it start from the copy in HBM"""
    def __init__(self, ctx, vars_):
        self.n = len(vars_) // 4
        self.h = _chk(H.spz_vars_assignment_new(ctx.h, vars_, sz(self.n)), "VarsAssignment::new")

    @classmethod
    def _resident(cls, h):
        a = cls.__new__(cls)
        a.h = vp(h)
        a.n = int(H.spz_vars_assignment_len(a.h))
        return a

    @classmethod
    def from_bytes(cls, ctx, data):
        """Assignment::new (lib.rs:62-88) as the reference takes it: `data` is any buffer of 32 n bytes (bytes, bytearray, memoryview, a NumPy
        uint8 array), n canonical little-endian scalars. The bytes are uploaded as they are; the comparison with q and the conversion to
        Montgomery form run on the device. Raises InvalidScalar when an entry is >= q."""
        what = "VarsAssignment::from_bytes"
        buf, n = _byte_buffer(data, what)
        rep = (ctypes.c_uint64 * 2)()
        h = H.spz_vars_assignment_from_bytes(ctx.h, buf, sz(n), rep)
        _scalar_result(h, rep, what)
        return cls._resident(h)

    @classmethod
    def from_tensor(cls, ctx, t):
        """The same from a torch.uint8 tensor of 32 n elements on the context's device, read through its data_ptr(): the witness never visits
        host memory. The tensor must be contiguous; it may be a view at any byte offset. THE CALLER SYNCHRONISES the stream that wrote the
        tensor before the call (torch.cuda.synchronize(), or a synchronize of that stream): the library copies on its own stream, which is
        not ordered against torch's. Raises InvalidScalar when an entry is >= q."""
        import torch
        from .capi import lib
        what = "VarsAssignment::from_tensor"
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
            raise SpartanHipError(f"{what}: a torch.uint8 tensor on the GPU is required")
        dev = int(lib.sp_ctx_device(ctx.raw()))
        if t.device.index != dev:
            raise SpartanHipError(f"{what}: the tensor is on device {t.device.index}, the context on device {dev}")
        if not t.is_contiguous():
            raise SpartanHipError(f"{what}: the tensor is not contiguous")
        if t.numel() == 0 or t.numel() % 32:
            raise SpartanHipError(f"{what}: {t.numel()} bytes are not a whole, non-zero number of 32-byte scalars")
        rep = (ctypes.c_uint64 * 2)()
        h = H.spz_vars_assignment_from_device_bytes(ctx.h, vp(t.data_ptr()), sz(t.numel() // 32), rep)
        _scalar_result(h, rep, what)
        return cls._resident(h)

    def to_bytes(self):
        """Scalar::to_bytes of every entry: 32 n canonical little-endian bytes"""
        out = (ctypes.c_uint8 * (32 * self.n))()
        if H.spz_vars_assignment_to_bytes(self.h, out) != 0:
            raise SpartanHipError(_failed("VarsAssignment::to_bytes"))
        return bytes(out)

    def check_reduced(self):
        """(count, first): how many of the resident entries have limbs >= q and the lowest such index (None when count is 0). An assignment made
        from bytes is reduced by construction; one made from Montgomery limbs is taken on trust, and this is the check of that trust."""
        rep = (ctypes.c_uint64 * 2)()
        if H.spz_vars_assignment_check_reduced(self.h, rep) != 0:
            raise SpartanHipError(_failed("VarsAssignment::check_reduced"))
        return int(rep[0]), (int(rep[1]) if rep[0] else None)

    def free(self):
        if self.h:
            H.spz_vars_assignment_free(self.h); self.h = None


class InputsAssignment:
    """InputsAssignment::new (lib.rs:56-105) for the few public inputs: parsed on the calling thread, no context"""
    @staticmethod
    def from_bytes(data):
        """32 n canonical little-endian bytes -> the ctypes uint64 array of Montgomery limbs that every `inputs` parameter takes.
        Raises InvalidScalar when an entry is >= q."""
        what = "InputsAssignment::from_bytes"
        buf, n = _byte_buffer(data, what)
        limbs = (ctypes.c_uint64 * (4 * n))()
        rep = (ctypes.c_uint64 * 2)()
        _scalar_result(H.spz_scalars_from_bytes(buf, sz(n), limbs, rep) == 0, rep, what)
        return limbs

    @staticmethod
    def to_bytes(limbs):
        """Scalar::to_bytes of each input: Montgomery limbs (a ctypes uint64 array) -> 32 n canonical little-endian bytes"""
        n = len(limbs) // 4
        out = (ctypes.c_uint8 * (32 * n))()
        if H.spz_scalars_to_bytes(limbs, sz(n), out) != 0:
            raise SpartanHipError(_failed("InputsAssignment::to_bytes"))
        return bytes(out)


class Encoded:
    def __init__(self, h):
        self.h = h

    def comm(self, which):
        return _fill(H.spz_encode_comm, self.h, which, unit=32)   # this one counts points

    def serialize_commitment(self):
        return _fill(H.spz_commitment_bincode, self.h)

    def commitment(self, ctx):
        """the Commitment a verifier would load from serialize_commitment()"""
        return Commitment.load(ctx, self.serialize_commitment())

    def serialize_decommitment(self):
        return _fill(H.spz_decommitment_bincode, self.h)

    def free(self):
        if self.h:
            H.spz_encode_free(self.h); self.h = None
