// Host half of what a caller had to compose before sp_r1cs_check existed (bench/is_sat_probe.py, leg b): after three sp_sparse_mulvec and three
// sp_table_download, the loop of Montgomery multiplications over the downloaded tables. The field code is the library's own, compiled for the host.
//   g++ -O2 -std=c++17 -fPIC -shared bench/is_sat_host.cc -o bench/is_sat_host.so
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../spartan_amd/csrc/field.hpp"

using namespace sp;

extern "C" size_t isat_host_count(const uint64_t* az, const uint64_t* bz, const uint64_t* cz, size_t n) {  // rows with Az * Bz != Cz
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    Fq a, b, c;
    memcpy(a.l, az + 4 * i, 32); memcpy(b.l, bz + 4 * i, 32); memcpy(c.l, cz + 4 * i, 32);
    bad += !fq_eq(fq_mul(a, b), c);
  }
  return bad;
}
