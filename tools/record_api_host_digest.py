#!/usr/bin/env python3
"""Record tests/golden/api_host/digest.txt from the code that csrc/pqgpu_api_host.cpp was moved out of
(DESIGN.md §2c).

It takes csrc/pqgpu_api.hip of COMMIT (default: the last commit that held these functions) out of git and
cuts out, as text: router_hit, the body of pqg_router_cache_lookup, the stream walk of pqg_router_read_page
(from its `const uint64_t L = stream_left` to `c.misses++`), the body of resolve_page_errors, the epoch loop
of resolve_errors and the prefix loop of dict_page_eof_code. None of them makes a HIP call. Each is compiled
for the host behind the signature pqgpu_api_host.h gives it today (a stand-in context, plan and status
supply the names the old text uses) and linked with tests/c/api_host_main.cpp, so that the same case list is
printed by the same routine. The functions that are in no digest line (router_runs_*) come from today's
pqgpu_api_host.cpp. Nothing of the scratch build is kept.

    tools/record_api_host_digest.py [--commit COMMIT] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "parquet-mr_amd", "csrc")
MOVED = ["router_hit", "router_cache_lookup", "router_walk", "decode_error_words", "resolve_page_errors",
         "dict_page_eof_code"]

OLD_CORE = r"""
#include <algorithm>
#include <cstring>

#include "%(host_h)s"

namespace pqg {

%(router_hit)s

int router_cache_lookup(RouterCache* c, int bit_width, const uint8_t* run, size_t stream_left, int count, int32_t* out,
                        int* hit) {
  struct Ctx { RouterCache& router; };
  RouterCache none;
  Ctx have{c ? *c : none};
  Ctx* ctx = c ? &have : nullptr;
%(lookup_body)s
}

void router_walk(RouterCache& c, int bit_width, const uint8_t* in, uint64_t stream_left, int count) {
%(walk)s
}

void decode_error_words(std::vector<uint64_t>* words, uint32_t epoch) {
  struct { uint32_t err_epoch; } plan{epoch}, *P = &plan;
  std::vector<uint64_t>& errs = *words;
%(decode)s
}

namespace {
struct OldPlan { const PlanLayout& L; std::vector<pqg_page_error>& page_errs; };
struct OldStatus { bool set; int page; int64_t idx; const char* what; };
void set_status(OldStatus* st, int, int page, int64_t idx, const char* what) { *st = OldStatus{true, page, idx, what}; }
int old_resolve_page_errors(OldPlan* P, OldStatus* st, const std::vector<uint64_t>& errs) {
%(resolve_body)s
}
}  // namespace

int resolve_page_errors(const PlanLayout& L, const std::vector<uint64_t>& errs, std::vector<pqg_page_error>* page_errs,
                        int* first_page, int64_t* index, const char** what) {
  OldPlan P{L, *page_errs};
  OldStatus st{false, -1, -1, nullptr};
  const int rc = old_resolve_page_errors(&P, &st, errs);
  if (st.set) { *first_page = st.page; *index = st.idx; *what = st.what; }
  return rc;
}

int dict_page_eof_code(const uint8_t* bytes, size_t size, uint32_t n_values) {
  std::vector<uint8_t> page(bytes, bytes + size);
  struct { uint32_t dict_num_values; } user{n_values};
%(dict_loop)s
}

}  // namespace pqg
"""


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr, flush=True)
    return subprocess.run(cmd, check=True, **kw)


def between(src, start, end, at=0, keep_start=True):
    """The text from `start` (first occurrence at or after `at`) up to and including `end`."""
    i = src.index(start, at)
    j = src.index(end, i + len(start)) + len(end)
    return src[i if keep_start else i + len(start):j]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default="4bee318")
    ap.add_argument("--out", default=None, help="default: standard output")
    args = ap.parse_args()
    src = run(["git", "-C", REPO, "show", args.commit + ":parquet-mr_amd/csrc/pqgpu_api.hip"], capture_output=True,
              text=True).stdout
    end_fn = "\n}\n"  # a function's closing brace (the bodies below hold no other brace in column 0)
    parts = {
        "host_h": os.path.join(CSRC, "pqgpu_api_host.h"),
        "router_hit": between(src, "bool router_hit(RouterCache& c,", end_fn),
        "lookup_body": between(src, "int* hit) {\n", end_fn, src.index("int pqg_router_cache_lookup("), keep_start=False)[:-2],
        "walk": between(src, "  const uint64_t L = stream_left, need", "  c.misses++;\n", src.index("int pqg_router_read_page(")),
        "decode": between(src, "    for (uint64_t& w : errs)", ": ~0ull;\n"),
        "resolve_body": between(src, "const std::vector<uint64_t>& errs) {\n", end_fn,
                                src.index("\nint resolve_page_errors(pqg_plan* P, pqg_status* st, const std::vector<uint64_t>& errs) {"),
                                keep_start=False)[:-2],
        "dict_loop": between(src, "  uint64_t p = 0;\n", "  return PQG_ERR_EOF;\n", src.index("static int dict_page_eof_code(")),
    }
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "old_core.cpp"), "w") as f:
            f.write(OLD_CORE % parts)
        exe = os.path.join(tmp, "api_host_old")
        flags = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "include")]
        run(flags + ["-c", os.path.join(tmp, "old_core.cpp"), "-o", os.path.join(tmp, "old_core.o")])
        # today's file with the moved functions renamed out of the way: what is left is router_runs_*
        run(flags + ["-D%s=unused_new_%s" % (n, n) for n in MOVED] +
            ["-c", os.path.join(CSRC, "pqgpu_api_host.cpp"), "-o", os.path.join(tmp, "rest.o")])
        run(flags + [os.path.join(REPO, "tests", "c", "api_host_main.cpp"), os.path.join(tmp, "old_core.o"),
                     os.path.join(tmp, "rest.o"), "-o", exe])
        run([exe, "cases"], capture_output=True)  # the old code passes the cases' own checks too
        out = run([exe, "digest"], capture_output=True, text=True).stdout
    if args.out:
        with open(args.out, "w") as f:
            f.write(out)
    else:
        sys.stdout.write(out)


if __name__ == "__main__":
    main()
