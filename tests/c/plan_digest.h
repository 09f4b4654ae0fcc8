// plan_digest.h — one text line per pqg::PlanLayout: every scalar in the order of line() below (values
// only, to keep the recorded file small), then <entries>:<64-bit FNV-1a hash> of every table ("-": empty).
// tests/c/plan_layout.cpp hashes these lines into tests/golden/plan/layout_digest.txt (one 64-bit hash per
// distinct layout of a case) and prints them in its digest-full mode; whatever records that file prints
// through the same routine. The region table (names) is not part of the digest: only the
// offsets it produced are.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "../../parquet-mr_amd/csrc/pqgpu_plan.h"

namespace plan_digest {

inline uint64_t fnv(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

template <class T>
uint64_t hash_vec(const std::vector<T>& v) {
  return fnv(v.data(), sizeof(T) * v.size());  // (T without padding bytes)
}

inline std::string line(const pqg::PlanLayout& L) {
  std::string s;
  char b[96];
  auto num = [&](const char* k, uint64_t v) {
    (void)k;
    std::snprintf(b, sizeof(b), " %llu", (unsigned long long)v);
    s += b;
  };
  auto hash = [&](const char* k, uint64_t v, size_t n) {
    (void)k;
    if (n) std::snprintf(b, sizeof(b), " %zu:%016llx", n, (unsigned long long)v);
    s += n ? b : " -";
  };
#define PD_NUM(f) num(#f, (uint64_t)L.f)
#define PD_ARR(f, n) for (int i_ = 0; i_ < (n); i_++) num(#f, (uint64_t)L.f[i_])
#define PD_VEC(f) hash(#f, hash_vec(L.f), L.f.size())
  PD_NUM(n_pages); PD_NUM(n_cols); PD_NUM(rec_total); PD_NUM(chunk_total); PD_NUM(scratch_bytes);
  PD_NUM(blen_bytes); PD_NUM(blen_bytes_nf);
  PD_ARR(chunk_off, pqg::N_DICT_CLS); PD_ARR(chunk_n, pqg::N_DICT_CLS);
  PD_ARR(dd_chunk_off, 2); PD_ARR(dd_chunk_n, 2); PD_NUM(dd_region); PD_ARR(dd_sums_off, 2);
  PD_ARR(n_dd_cols, 2); PD_ARR(off_dd_cols, 2); PD_ARR(off_dd_start, 2);
  PD_NUM(n_dict_walk); PD_NUM(n_bind); PD_NUM(n_fixd); PD_NUM(n_bin_cols); PD_NUM(n_carry);
  PD_NUM(off_dict_walk); PD_NUM(off_bind); PD_NUM(off_fixd); PD_NUM(off_bin_cols); PD_NUM(off_carry);
  PD_NUM(n_dent_tiles); PD_NUM(n_dent_cols); PD_NUM(off_dent_cols); PD_NUM(off_dent_start);
  PD_NUM(dent_rec_off); PD_NUM(dent_scr_off); PD_NUM(dent_tb_off);
  PD_NUM(n_bin_blocks); PD_NUM(n_bin_chunks); PD_NUM(n_dba_chunks); PD_NUM(dba_meta_off);
  PD_ARR(cls_off, pqg::C_NCLS); PD_ARR(cls_n, pqg::C_NCLS);
  PD_NUM(levels_off); PD_NUM(levels_n); PD_NUM(n_scan_cols);
  PD_NUM(n_segs); PD_NUM(seg_status_off); PD_NUM(seg_tmp_off);
  PD_NUM(plain_pg); PD_NUM(n_pcp); PD_NUM(n_psegs); PD_NUM(n_pcols); PD_NUM(pticket_off); PD_NUM(pflag_off);
  PD_NUM(n_binp_fused); PD_NUM(n_bin_cols_nf); PD_NUM(n_binp_seg); PD_NUM(n_bin_blocks_nf); PD_NUM(n_bin_chunks_nf);
  PD_NUM(null_hints); PD_NUM(hint_off);
  s += " |";
  PD_VEC(h_work); PD_VEC(cols); PD_VEC(flat); PD_VEC(cp); PD_VEC(cps); PD_VEC(bl);
  PD_VEC(bin_blocks); PD_VEC(bin_chunks); PD_VEC(dba_chunks); PD_VEC(segs); PD_VEC(dent_tiles); PD_VEC(psegs);
  PD_VEC(pcp); PD_VEC(pcs); PD_VEC(chunk_list);
  PD_VEC(blen_off); PD_VEC(bsrc_off); PD_VEC(dlen_off); PD_VEC(dsrc_off); PD_VEC(dent_off); PD_VEC(bsum_off);
  PD_VEC(bin_total_off);
  PD_VEC(page_cls); PD_VEC(col_nullable); PD_VEC(col_required_values); PD_VEC(col_first_page); PD_VEC(bin_capacity);
  PD_VEC(empty_bin_values);
#undef PD_NUM
#undef PD_ARR
#undef PD_VEC
  uint64_t h = 0xcbf29ce484222325ull;
  for (const pqg::HostErr& e : L.host_errs) {  // (field by field: the struct has padding)
    const int64_t f[4] = {e.page, e.kind, e.index, e.code};
    h = fnv(f, sizeof(f), h);
  }
  hash("host_errs", h, L.host_errs.size());
  return s;
}

}  // namespace plan_digest
