"""GPU ZSTD decompression (pqg_zstd_decompress, csrc/pqgpu_zstd.hip) on hand-built frames
(zstd_build.py, zstd_cases.py; tests/test_zstd_build.py holds every one of them against libzstd):
constructs libzstd's encoder never or rarely emits, at the sizes where the kernel takes another
path. Every legal group runs with the sequence pre-pass (k_zstd_seq + replay) and without it
(PQG_DISPATCH_ZSTD_PREPASS 0: the inline decoder zseq_decode, otherwise only the pre-pass's
fallback). Illegal frames must be reported with the oracle's code, beside intact legal neighbours."""
import numpy as np
import pytest

from oracle import pqref
from pqgpu import abi, native

from zstd_cases import GROUPS, illegal_cases, legal_cases

pytestmark = pytest.mark.gpu
POISON = 0xA5  # the decoder fixture's poison byte: what unwritten output holds
GUARD = 16  # bytes between two jobs' outputs (Decoder.zstd_decompress)


def _run(decoder, cases, prepass):
    """One pqg_zstd_decompress call for all `cases` -> per case (status, output bytes, guard bytes)."""
    assert decoder.poison == POISON
    decoder.set_dispatch(abi.DISPATCH_ZSTD_PREPASS, prepass)
    try:
        out, offs, status, _ = decoder.zstd_decompress([c.frame for c in cases], [c.n for c in cases])
    finally:
        decoder.set_dispatch(abi.DISPATCH_ZSTD_PREPASS, 1)
    host = out.cpu().numpy()
    return [(int(status[i]), host[offs[i]:offs[i] + c.n].tobytes(), host[offs[i] + c.n:offs[i] + c.n + GUARD].tobytes())
            for i, c in enumerate(cases)]


def _check_legal(cases, got):
    bad = []
    for c, (st, data, guard) in zip(cases, got):
        if st != 0:
            bad.append((c.id, "status", st))
        elif data != c.expected[:c.n]:
            diff = next(i for i in range(c.n) if data[i] != c.expected[i])
            bad.append((c.id, "first wrong byte", diff, "of", c.n))
        elif guard != bytes([POISON]) * GUARD:
            bad.append((c.id, "wrote past its output"))
    assert not bad, bad


@pytest.mark.parametrize("prepass", [1, 0], ids=["prepass", "inline"])
@pytest.mark.parametrize("group", GROUPS)
def test_legal_frames(decoder, group, prepass):
    cases = [c for c in legal_cases() if c.group == group]
    assert cases
    _check_legal(cases, _run(decoder, cases, prepass))


@pytest.mark.parametrize("prepass", [1, 0], ids=["prepass", "inline"])
def test_illegal_frames(decoder, prepass):
    """legal, illegal, legal, illegal, ..., legal in one call: every illegal frame gets the oracle's
    error code and leaves the bytes past its output alone; its neighbours decode as if alone."""
    legal = [c for c in legal_cases() if c.group in ("tables", "repeat-offsets")]
    cases = []
    for i, c in enumerate(illegal_cases()):
        cases += [legal[i % len(legal)], c]
    cases.append(legal[-1])
    got = _run(decoder, cases, prepass)
    _check_legal(cases[0::2], got[0::2])
    bad = []
    for c, (st, _, guard) in zip(cases[1::2], got[1::2]):
        try:
            pqref.zstd_decompress(c.frame, c.n)
            want = 0
        except ValueError as e:
            want = int(str(e).split("error ")[1])
        assert want == abi.ERR_CORRUPT, c.id
        if st != want:
            bad.append((c.id, "status", st))
        elif guard != bytes([POISON]) * GUARD:
            bad.append((c.id, "wrote past its output"))
    assert not bad, bad


def test_prepass_key_is_validated(decoder):
    with pytest.raises(native.PqgError) as e:
        decoder.set_dispatch(abi.DISPATCH_ZSTD_PREPASS, 2)
    assert e.value.code == abi.ERR_INVALID_ARG
    decoder.set_dispatch(abi.DISPATCH_ZSTD_PREPASS, 1)
