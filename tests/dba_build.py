"""Hand-built DELTA_BYTE_ARRAY pages: a page builder, an independent reader and a model of the copy's
dispatch.

page() writes a data section from prefix lengths and suffixes that the caller chooses freely (the
prefix need not be the common prefix of consecutive values, and need not be legal); both length streams
come from delta_build / delta_cases.int_stream, in any block / miniblock shape. It does not use
tools/synth/writer.py's dba_encode.

unroll() is DeltaByteArrayReader.readBytes (parquet-column/.../deltastrings/DeltaByteArrayReader.java
:57-79) in Python bytes: value i = previous[:prefix_i] + suffix_i. It calls neither the oracle nor the
kernels: it is the expected output by construction, and the second opinion on oracle/pqref.c.

paths() restates, from the lengths alone, which way the value copy of csrc/pqgpu_binary.hip sends a
page (k_dba_copy / k_dba_tail / k_dba_chain_par / k_dba_chain / k_dba_chunks, dba_values, dba_batch),
so that a test can assert that a case reaches the seam it is named for. The six constants below are
the kernels'; tests/test_dba_build.py checks them against the sources.
"""
import numpy as np

import delta_cases as DC

WAVE = 64         # values per batch (pqgpu_device.h)
BIN_CHUNK = 256   # values per chunk (pqgpu_plan.h)
DCP = 256         # chunks per page of k_dba_chain_par; more: k_dba_chain (pqgpu_binary.hip)
DBA_VB = 2048     # longest value of a chunk-parallel page (pqgpu_internal.h)
DBA_SB = 3072     # staged suffix bytes per chunk / batch (pqgpu_binary.hip)
DBA_OB = 4096     # assembled bytes of a byte-parallel batch (pqgpu_binary.hip)

# where each constant is declared: (file under parquet-mr_amd/csrc, name, value)
CONSTANTS = [("pqgpu_device.h", "WAVE", WAVE), ("pqgpu_plan.h", "BIN_CHUNK", BIN_CHUNK),
             ("pqgpu_binary.hip", "DCP", DCP), ("pqgpu_internal.h", "DBA_VB", DBA_VB),
             ("pqgpu_binary.hip", "DBA_SB", DBA_SB), ("pqgpu_binary.hip", "DBA_OB", DBA_OB)]


# ---- builder ------------------------------------------------------------------------------------------

def page(prefixes, suffixes, prefix_cfg=(128, 4), suffix_cfg=(128, 4), seed=0):
    """The data section: prefix lengths, suffix lengths (both DELTA_BINARY_PACKED), suffix bytes."""
    assert len(prefixes) == len(suffixes)
    rng = np.random.default_rng(seed)
    return DC.int_stream(rng, *prefix_cfg, [int(p) for p in prefixes], wide=False) + \
        DC.int_stream(rng, *suffix_cfg, [len(s) for s in suffixes], wide=False) + b"".join(suffixes)


# ---- reader -------------------------------------------------------------------------------------------

class Illegal(Exception):
    """The reference reader throws at value `index` (kind: "prefix" or "eof")."""

    def __init__(self, index, kind):
        super().__init__(f"{kind} at value {index}")
        self.index, self.kind = index, kind


def unroll(prefixes, suffixes, previous=b"", suffix_bytes=None):
    """readBytes x n: value i = previous[:p_i] + s_i. Raises Illegal at the first value whose prefix
    is negative or longer than the previous value (System.arraycopy :72 throws), or, with
    suffix_bytes (the bytes the page holds after the two length streams), whose suffix ends past
    them (the suffix reader's slice throws first)."""
    out, used = [], 0
    for i, (p, s) in enumerate(zip(prefixes, suffixes)):
        used += len(s)
        if suffix_bytes is not None and used > suffix_bytes:
            raise Illegal(i, "eof")
        if p != 0:
            if p < 0 or p > len(previous):
                raise Illegal(i, "prefix")
            previous = previous[:p] + s
        else:
            previous = s
        out.append(previous)
    return out


# ---- the dispatch, from the lengths ----------------------------------------------------------------------

def copy_prefix(prefixes, lengths, i):
    """The prefix k_delta stores for the copy: an empty value's is 0."""
    return prefixes[i] if lengths[i] else 0


def paths(prefixes, lengths):
    """A legal page's way through the copy.

    -> dict(serial, n_chunks, chunks=[...], batches=[...])
    serial: a value longer than DBA_VB (the whole page goes to k_dba_copy).
    chunks[c]: suffix (suffix bytes of the chunk), m (smallest copy prefix in it: an empty value
      counts as prefix 0, as k_delta stores it), last_len (length of the chunk's last value T_c),
      inherited (for each byte b < min(m, last_len) of T_c: how many chunks back its donor chunk
      is, i.e. the last earlier chunk whose values wrote byte b) and own (for each byte b >= m of
      T_c: how many values before the chunk's last value its donor value is).
    batches[k] (64 values from the chunk's start): total (assembled bytes), suffix (suffix bytes),
      depth (longest chain of previous-smaller links that stay inside the batch: dba_batch's loop).
    The donors come from replaying the writes (who wrote byte b last), not from the kernels' formula.
    """
    n = len(prefixes)
    assert n == len(lengths)
    n_chunks = (n + BIN_CHUNK - 1) // BIN_CHUNK
    out = dict(serial=max(lengths, default=0) > DBA_VB, n_chunks=n_chunks, chunks=[], batches=[])
    owner = []  # owner[b]: index of the value that wrote byte b of the current value
    for c in range(n_chunks):
        lo, hi = c * BIN_CHUNK, min((c + 1) * BIN_CHUNK, n)
        for i in range(lo, hi):
            p, ln = prefixes[i], lengths[i]
            assert 0 <= p <= len(owner) and p <= ln, (i, p, ln, len(owner))
            owner[p:] = [i] * (ln - p)
        m = min(copy_prefix(prefixes, lengths, i) for i in range(lo, hi))
        last = hi - 1
        k = min(m, lengths[last])
        inherited = [c - owner[b] // BIN_CHUNK for b in range(k)]
        own = [last - owner[b] for b in range(k, lengths[last])]
        assert all(d >= 1 for d in inherited) and all(0 <= d < BIN_CHUNK for d in own)
        out["chunks"].append(dict(suffix=sum(lengths[i] - prefixes[i] for i in range(lo, hi)), m=m,
                                  last_len=lengths[last], inherited=inherited, own=own))
        for b0 in range(lo, hi, WAVE):
            b1 = min(b0 + WAVE, hi)
            depth, stack, best = {}, [], 0
            for i in range(b0, b1):
                p = copy_prefix(prefixes, lengths, i)
                while stack and copy_prefix(prefixes, lengths, stack[-1]) >= p:
                    stack.pop()
                depth[i] = depth[stack[-1]] + 1 if (stack and p > 0) else 0
                best = max(best, depth[i])
                stack.append(i)
            out["batches"].append(dict(total=sum(lengths[b0:b1]), suffix=sum(lengths[i] - prefixes[i] for i in range(b0, b1)),
                                       depth=best))
    return out

