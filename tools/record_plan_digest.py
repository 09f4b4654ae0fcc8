#!/usr/bin/env python3
"""Record tests/golden/plan/layout_digest.txt from the arithmetic plan creation had before the planner was
moved to csrc/pqgpu_plan_host.cpp, or print that arithmetic's full digest lines to compare
with `plan_layout digest-full` when a hash differs.

It takes csrc/pqgpu_api.hip of COMMIT (default: the last commit that held plan_create_impl whole) out of
git into a scratch directory, deletes plan_create_impl's hipSetDevice line, makes the function return just
before its `// ---- upload` line after copying its locals and plan fields into a pqg::PlanLayout, compiles
that for the host behind the signature of pqg::plan_layout (a bare pqg_ctx; libamdhip64 loads without a
device and no HIP call is reached) and links it with tests/c/plan_layout.cpp, so that the same case list is
printed by the same routine. Nothing of the scratch build is kept.

    tools/record_plan_digest.py [--commit COMMIT] [--mode digest|digest-full] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SET_DEVICE = "  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;\n"

# Inserted before `// ---- upload`. The loop applies the lines of the commit's pointer-resolution block that
# do not depend on the allocation, as that commit applies them after it.
CAPTURE = r"""
  {
    NewLayout& L = *g_out;
    L = NewLayout();
    L.n_pages = n_pages; L.n_cols = n_cols;
    for (int i = 0; i < n_cols; i++) {
      ColumnDev& d = hc[(size_t)i];
      d.blen = ids_mode(cols[i]) ? (uint32_t*)cols[i].values : nullptr;
      d.n_slots = slot_acc[(size_t)i];
      d.dict_direct = dict_direct[(size_t)i] ? (cols[i].dict_num_values <= 256 && !dd_glob[(size_t)i] ? 1u : 2u) : 0u;  // id bytes
      d.dd_global = dd_glob[(size_t)i];
      if (dba_fixed[(size_t)i]) {  // DELTA_BYTE_ARRAY values go straight to the fixed-width output
        d.binary_data = (uint8_t*)cols[i].values;
        d.binary_capacity = slot_acc[(size_t)i] * (uint64_t)d.elem_width;
      }
    }
    static_assert(sizeof(ColumnDev) == sizeof(NewColumnDev) && sizeof(PageWork) == sizeof(NewPageWork), "layout");
    L.h_work.resize(P->h_work.size()); std::memcpy(L.h_work.data(), P->h_work.data(), sizeof(PageWork) * P->h_work.size());
    L.cols.resize(hc.size()); std::memcpy(L.cols.data(), hc.data(), sizeof(ColumnDev) * hc.size());
    L.flat = flat; L.cp = cp; L.cps = cps; L.bl = bl; L.bin_blocks = bin_blocks; L.bin_chunks = bin_chunks;
    L.dba_chunks = dba_chunks; L.segs = segs; L.dent_tiles = dent_tiles; L.psegs = psegs; L.pcp = pcp; L.pcs = pcs;
    L.chunk_list = chunk_list;
    L.rec_total = rec_total; L.chunk_total = chunk_total; L.scratch_bytes = sc;
    L.blen_off = blen_off; L.bsrc_off = bsrc_off; L.dlen_off = dlen_off; L.dsrc_off = dsrc_off; L.dent_off = dent_off;
    L.bsum_off = bsum_off; L.bin_total_off = P->bin_total_off;
    L.blen_bytes = P->blen_bytes; L.blen_bytes_nf = P->blen_bytes_nf;
    for (int i = 0; i < 3; i++) { L.chunk_off[i] = P->chunk_off[i]; L.chunk_n[i] = P->chunk_n[i]; }
    for (int g = 0; g < 2; g++) {
      L.dd_chunk_off[g] = P->dd_chunk_off[g]; L.dd_chunk_n[g] = P->dd_chunk_n[g]; L.dd_sums_off[g] = P->dd_sums_off[g];
      L.n_dd_cols[g] = P->n_dd_cols[g]; L.off_dd_cols[g] = P->off_dd_cols[g]; L.off_dd_start[g] = P->off_dd_start[g];
    }
    L.dd_region = P->dd_region;
    L.n_dict_walk = P->n_dict_walk; L.n_bind = P->n_bind; L.n_fixd = P->n_fixd; L.n_bin_cols = P->n_bin_cols; L.n_carry = P->n_carry;
    L.off_dict_walk = P->off_dict_walk; L.off_bind = P->off_bind; L.off_fixd = P->off_fixd; L.off_bin_cols = P->off_bin_cols;
    L.off_carry = P->off_carry;
    L.n_dent_tiles = P->n_dent_tiles; L.n_dent_cols = P->n_dent_cols; L.off_dent_cols = P->off_dent_cols;
    L.off_dent_start = P->off_dent_start; L.dent_rec_off = P->dent_rec_off; L.dent_scr_off = P->dent_scr_off; L.dent_tb_off = P->dent_tb_off;
    L.n_bin_blocks = P->n_bin_blocks; L.n_bin_chunks = P->n_bin_chunks; L.n_dba_chunks = P->n_dba_chunks; L.dba_meta_off = P->dba_meta_off;
    for (int k = 0; k < C_NCLS; k++) { L.cls_off[k] = P->cls_off[(size_t)k]; L.cls_n[k] = P->cls_n[(size_t)k]; }
    L.levels_off = P->levels_off; L.levels_n = P->levels_n; L.n_scan_cols = P->n_scan_cols;
    L.n_segs = P->n_segs; L.seg_status_off = P->seg_status_off; L.seg_tmp_off = P->seg_tmp_off;
    L.plain_pg = P->plain_pg;
    // (the commit sets these three after the upload, from the same vectors)
    L.n_pcp = (int)pcp.size(); L.n_psegs = (uint32_t)psegs.size(); L.n_pcols = (int)pcs.size() - 1;
    L.pticket_off = P->pticket_off; L.pflag_off = P->pflag_off;
    L.n_binp_fused = P->n_binp_fused; L.n_bin_cols_nf = P->n_bin_cols_nf; L.n_binp_seg = P->n_binp_seg;
    L.n_bin_blocks_nf = P->n_bin_blocks_nf; L.n_bin_chunks_nf = P->n_bin_chunks_nf;
    L.null_hints = P->null_hints; L.hint_off = P->hint_off;
    L.page_cls = P->page_cls; L.col_nullable = P->col_nullable; L.col_required_values = P->col_required_values;
    L.col_first_page = P->col_first_page; L.bin_capacity = P->bin_capacity; L.empty_bin_values = P->empty_bin_values;
    for (const HostErr& e : P->host_errs) L.host_errs.push_back(NewHostErr{e.page, e.kind, e.index, e.code});
    delete P;
    return PQG_OK;
  }
"""

# The commit's namespace pqg becomes pqg_old, so that its ColumnDev / PageWork and today's can share a file.
DRIVER = r"""
#include "%(plan_h)s"
using NewLayout = pqg::PlanLayout; using NewColumnDev = pqg::ColumnDev; using NewPageWork = pqg::PageWork;
using NewHostErr = pqg::HostErr;
static NewLayout* g_out;
#define pqg pqg_old
#include "old_api.inc"
#undef pqg
namespace pqg {
int old_plan_layout(uint64_t n_bytes, uint64_t valid_bytes, const pqg_column_desc* cols, int n_cols,
                    const pqg_page_desc* pages, int n_pages, const PlanOptions& opt, PlanLayout* out, int* bad_page) {
  pqg_ctx ctx;  // bare: no device, no stream
  ctx.plain_mode = opt.plain_mode; ctx.dict_direct = opt.dict_direct; ctx.null_hints = opt.null_hints;
  g_out = out;
  pqg_plan* P = nullptr;
  pqg_status st;
  const int rc = plan_create_impl(&ctx, (const uint8_t*)0x100000, n_bytes, valid_bytes, cols, n_cols, pages, n_pages, &P, &st);
  *bad_page = rc == PQG_OK ? -1 : st.page;
  return rc;
}
// the commit's count_kernels on one of its plans, filled from the layout
int plan_kernel_count(const PlanLayout& L, bool plain_fused, bool dict_fused, bool null_hints) {
  pqg_plan P;
  P.plain_fused = plain_fused; P.dict_fused = dict_fused; P.null_hints = null_hints;
  P.levels_n = L.levels_n; P.n_scan_cols = L.n_scan_cols;
  P.cls_n.assign(L.cls_n, L.cls_n + C_NCLS);
  P.n_binp_seg = L.n_binp_seg; P.n_binp_fused = L.n_binp_fused;
  P.n_dict_walk = L.n_dict_walk; P.n_dent_tiles = L.n_dent_tiles; P.n_bind = L.n_bind; P.n_fixd = L.n_fixd;
  P.n_bin_blocks = L.n_bin_blocks; P.n_bin_blocks_nf = L.n_bin_blocks_nf;
  P.n_bin_chunks = L.n_bin_chunks; P.n_bin_chunks_nf = L.n_bin_chunks_nf;
  P.n_dba_chunks = L.n_dba_chunks; P.n_carry = L.n_carry; P.n_segs = L.n_segs;
  return count_kernels(&P);
}
}  // namespace pqg
"""


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr, flush=True)
    return subprocess.run(cmd, check=True, **kw)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default="e617184")
    ap.add_argument("--mode", choices=["digest", "digest-full"], default="digest")
    ap.add_argument("--out", default=None, help="default: standard output")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = run(["git", "-C", REPO, "archive", args.commit, "parquet-mr_amd/csrc", "include"], capture_output=True).stdout
        run(["tar", "-x", "-C", tmp], input=tar)
        csrc = os.path.join(tmp, "parquet-mr_amd", "csrc")
        with open(os.path.join(csrc, "pqgpu_api.hip")) as f:
            src = f.read()
        i = src.index("static int plan_create_impl(")
        j = src.index(SET_DEVICE, i)
        src = src[:j] + src[j + len(SET_DEVICE):]
        k = src.index("  // ---- upload\n", i)
        src = src[:k] + CAPTURE + src[k:]
        with open(os.path.join(tmp, "old_api.inc"), "w") as f:
            f.write(src)
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER % {"plan_h": os.path.join(REPO, "parquet-mr_amd", "csrc", "pqgpu_plan.h")})
        exe = os.path.join(tmp, "plan_layout_old")
        run(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", csrc,
             "-c", os.path.join(tmp, "driver.cpp"), "-o", os.path.join(tmp, "driver.o")])
        run(["g++", "-std=c++17", "-O2", "-DPLAN_LAYOUT_CALL=old_plan_layout", "-I", os.path.join(REPO, "include"),
             "-c", os.path.join(REPO, "tests", "c", "plan_layout.cpp"), "-o", os.path.join(tmp, "cases.o")])
        # the kernel launchers the old file names are never reached: left unresolved
        run(["g++", os.path.join(tmp, "cases.o"), os.path.join(tmp, "driver.o"), "-o", exe, "-L", os.path.join(ROCM, "lib"),
             "-lamdhip64", "-Wl,--unresolved-symbols=ignore-all", "-Wl,-rpath," + os.path.join(ROCM, "lib")])
        out = run([exe, args.mode], capture_output=True, text=True).stdout
    if args.out:
        with open(args.out, "w") as f:
            f.write(out)
    else:
        sys.stdout.write(out)


if __name__ == "__main__":
    main()
