"""The byte layout of a bincode'd SNARK proof (lib.rs:311-316), walked from the struct definitions as tests/test_gpu_verify.py walks the NIZK's:
r1csproof.rs:21-37, sumcheck.rs:17-20 and 64-69, nizk/mod.rs:15-20, 77-81, 146-152, 292-299, 421-428, bullet.rs:15-19, dense_mlpoly.rs:38-41 and
303-306, product_tree.rs:133-139 and 162-166, sparse_mlpoly.rs:680-689, 1021-1028, 1307-1311, 1418-1422. bincode puts a u64 length in front of
every Vec and nothing else. Shared by tests/test_snark_parse.py (CPU) and tests/test_gpu_snark_verify.py; test infrastructure only."""


class Layout:
    """fields: {name: (offset, "scalar" | "point")} of every 32-byte field, the first element of a vector under its name and its last under
    name + ".last"; vectors: {name: (offset of the first element, number of elements, kind)}; lengths: [(offset of the u64 length, smallest
    encoding of one element, name)] of every Vec, outer and nested"""
    def __init__(self, p):
        self.p, self.o, self.fields, self.lengths, self.vectors = p, 0, {}, [], {}
        self._snark()
        assert self.o == len(p), (self.o, len(p))

    def _u64(self):
        return int.from_bytes(self.p[self.o:self.o + 8], "little")

    def _len(self, name, min_elem):
        k = self._u64()
        self.lengths.append((self.o, min_elem, name))
        self.o += 8
        return k

    def _vec(self, name, kind):
        k = self._len(name, 32)
        self.vectors[name] = (self.o, k, kind)
        if k:
            self.fields[name] = (self.o, kind)
            self.fields[name + ".last"] = (self.o + 32 * (k - 1), kind)
        self.o += 32 * k
        return k

    def _take(self, name, kind):
        self.fields[name] = (self.o, kind)
        self.o += 32

    def _zksc(self, tag):
        self._vec(tag + ".comm_polys", "point"); self._vec(tag + ".comm_evals", "point")
        for i in range(self._len(tag + ".proofs", 136)):
            t = "%s.proofs[%d]." % (tag, i)
            self._take(t + "delta", "point"); self._take(t + "beta", "point"); self._vec(t + "z", "scalar")
            self._take(t + "z_delta", "scalar"); self._take(t + "z_beta", "scalar")

    def _polyeval(self, tag):
        self._vec(tag + ".L_vec", "point"); self._vec(tag + ".R_vec", "point")
        self._take(tag + ".delta", "point"); self._take(tag + ".beta", "point"); self._take(tag + ".z1", "scalar"); self._take(tag + ".z2", "scalar")

    def _r1cs(self):
        self._vec("comm_vars", "point")
        self._zksc("sc1")
        for n in ("comm_Az", "comm_Bz", "comm_Cz", "comm_prod"):
            self._take("claims_phase2." + n, "point")
        self._take("pok.alpha", "point"); self._take("pok.z1", "scalar"); self._take("pok.z2", "scalar")
        self._take("prod.alpha", "point"); self._take("prod.beta", "point"); self._take("prod.delta", "point")
        for i in range(5):
            self._take("prod.z[%d]" % i, "scalar")
        self._take("eq1.alpha", "point"); self._take("eq1.z", "scalar")
        self._zksc("sc2")
        self._take("comm_vars_at_ry", "point")
        self._polyeval("eval_vars")
        self._take("eq2.alpha", "point"); self._take("eq2.z", "scalar")

    def _batched(self, tag):
        for i in range(self._len(tag + ".proof", 24)):
            t = "%s.proof[%d]." % (tag, i)
            for j in range(self._len(t + "compressed_polys", 8)):
                self._vec(t + "compressed_polys[%d]" % j, "scalar")
            self._vec(t + "claims_prod_left", "scalar"); self._vec(t + "claims_prod_right", "scalar")
        for w in ("left", "right", "weight"):
            self._vec(tag + ".claims_dotp_" + w, "scalar")

    def _snark(self):
        self._r1cs()
        for n in "ABC":
            self._take("inst_evals." + n, "scalar")
        self._vec("comm_derefs", "point")
        for side in ("row", "col"):
            self._take("prod_layer.%s_init" % side, "scalar"); self._vec("prod_layer.%s_read" % side, "scalar")
            self._vec("prod_layer.%s_write" % side, "scalar"); self._take("prod_layer.%s_audit" % side, "scalar")
        self._vec("prod_layer.eval_val_left", "scalar"); self._vec("prod_layer.eval_val_right", "scalar")
        self._batched("proof_mem"); self._batched("proof_ops")
        for side in ("row", "col"):
            self._vec("hash_layer.%s_addr" % side, "scalar"); self._vec("hash_layer.%s_read_ts" % side, "scalar")
            self._take("hash_layer.%s_audit_ts" % side, "scalar")
        self._vec("hash_layer.eval_val", "scalar"); self._vec("hash_layer.eval_row_ops_val", "scalar"); self._vec("hash_layer.eval_col_ops_val", "scalar")
        self._polyeval("hash_layer.proof_ops"); self._polyeval("hash_layer.proof_mem"); self._polyeval("hash_layer.proof_derefs")
