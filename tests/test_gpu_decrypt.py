"""Encrypted page modules on the device (pqg_decrypt_pages / pqg_decrypt_sync, Decoder.decrypt) against
tests/aes_ref.py (or the libcrypto it is pinned to, where there is one): random plaintext, modules built on the host
as BlockCipher.Encryptor writes them. The tile is forced to 1,024 bytes (PQG_DISPATCH_AES_TILE_BYTES), so that the
kernel's seams are cheap: its 16-byte lane blocks, its rows of 64 blocks = one tile here, several tiles per module,
more tiles than the fold has lanes."""
import ctypes as C

import numpy as np
import pytest
import torch

import aes_ref
from pqgpu import abi, native

pytestmark = pytest.mark.gpu
T = 1024
SIZES = [1, 15, 16, 17, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5, 4096 + 1]
BIG = (1 << 20) + 17
OFFSETS = [0, 1, 3, 8, 15]
AAD_LENGTHS = [13, 15, 16, 17, 31, 32, 200]
KEY_SIZES = [16, 24, 32]
CANARY = 0xC7
LIB = aes_ref.Libcrypto.load()


@pytest.fixture()
def small_tiles(decoder):
    decoder.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, T)
    yield decoder
    decoder.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, abi.AES_TILE_BYTES)


class Call:
    """The modules of one pqg_decrypt_pages call, laid out at chosen offsets mod 16 with gaps between them."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.src, self.rows, self.want, self.keys, self.aads = [], [], [], [], []
        self.src_pos = self.dst_pos = self.aad_pos = 0

    def key(self, size):
        self.keys.append(self.rng.bytes(size))
        return len(self.keys) - 1

    def add(self, mode, key, n, src_mod=0, dst_mod=0, aad_len=15, plain=None, nonce=None, aad=None):
        """Returns the job's index; the module is encrypted with keys[key]."""
        plain = self.rng.bytes(n) if plain is None else plain
        nonce = self.rng.bytes(12) if nonce is None else nonce
        aad = self.rng.bytes(aad_len) if aad is None else aad
        module = aes_ref.encrypt_module(self.keys[key], mode, nonce, plain, aad, backend=LIB)
        return self.add_module(mode, key, module, plain, aad, src_mod, dst_mod)

    def add_module(self, mode, key, module, plain, aad, src_mod=0, dst_mod=0):
        src = (self.src_pos + 15) // 16 * 16 + src_mod
        dst = (self.dst_pos + 15) // 16 * 16 + 16 + dst_mod  # at least 16 canary bytes before every range
        self.src.append((src, module))
        self.rows.append((src, dst, len(module), self.aad_pos, len(aad), mode, key, 0))
        self.want.append((dst, plain))
        self.aads.append(aad)
        self.src_pos, self.dst_pos, self.aad_pos = src + len(module), dst + len(plain), self.aad_pos + len(aad)
        return len(self.rows) - 1

    def run(self, decoder):
        """-> (status codes, pqg_decrypt_sync's rc, its status, the destination buffer as numpy)"""
        buf = self.rng.integers(0, 256, size=self.src_pos + 5, dtype=np.uint8)  # noise between the modules
        for off, m in self.src:
            buf[off:off + len(m)] = np.frombuffer(m, dtype=np.uint8)
        d_src = torch.from_numpy(buf).to(decoder.device)
        d_dst = torch.full((self.dst_pos + 32,), CANARY, dtype=torch.uint8, device=decoder.device)
        table = np.array(self.rows, dtype=abi.DECRYPT_JOB_DTYPE)
        codes, st = decoder.decrypt(d_src, d_dst, table, self.keys, b"".join(self.aads))
        return codes, st, d_dst.cpu().numpy()

    def check_output(self, out, skip=()):
        """Every plaintext byte for byte, and every byte outside the destination ranges still the canary."""
        mask = np.ones(out.size, dtype=bool)
        bad = []
        for j, (dst, plain) in enumerate(self.want):
            mask[dst:dst + len(plain)] = False
            if j not in skip and out[dst:dst + len(plain)].tobytes() != plain:
                bad.append((j, self.rows[j][:3], self.rows[j][5]))
        assert not bad, bad[:8]
        assert (out[mask] == CANARY).all(), np.flatnonzero(mask & (out != CANARY))[:8]


@pytest.mark.parametrize("key_size", KEY_SIZES)
@pytest.mark.parametrize("mode", [aes_ref.GCM, aes_ref.CTR], ids=["gcm", "ctr"])
def test_sizes_and_alignment(small_tiles, mode, key_size):
    """Every size at every (source, destination) offset pair mod 16; the AAD lengths in turn; two keys of the size."""
    c = Call(100 * key_size + mode)
    keys = [c.key(key_size), c.key(key_size)]
    n = 0
    for size in SIZES:
        for so in OFFSETS:
            for do in OFFSETS:
                c.add(mode, keys[n % 2], size, so, do, AAD_LENGTHS[n % len(AAD_LENGTHS)])
                n += 1
    assert n == len(SIZES) * 25
    codes, st, out = c.run(small_tiles)
    assert st.code == abi.OK and not codes.any(), (st.code, np.flatnonzero(codes)[:8])
    c.check_output(out)


@pytest.mark.parametrize("mode", [aes_ref.GCM, aes_ref.CTR], ids=["gcm", "ctr"])
def test_one_mebibyte_modules(small_tiles, mode):
    """1 MiB + 17: the counter's third byte carries, and 1,025 tiles are more than the fold has lanes. All key sizes,
    every source and destination offset once, jobs on different keys in one call."""
    c = Call(7 + mode)
    j = 0
    for k, key_size in enumerate(KEY_SIZES):
        key = c.key(key_size)
        for _ in range(2 if k else 1):
            c.add(mode, key, BIG, OFFSETS[j], OFFSETS[(j + 2) % 5], AAD_LENGTHS[j])
            j += 1
    assert j == len(OFFSETS)
    codes, st, out = c.run(small_tiles)
    assert st.code == abi.OK and not codes.any()
    c.check_output(out)


def test_default_tile_and_every_tile_size(decoder):
    """The default tile and each size the dispatch key takes: sizes around the tile, several tiles, all offsets."""
    try:
        for tile in (abi.AES_TILE_BYTES, 2048, 4096, 8192, 32768):
            decoder.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, tile)
            c = Call(tile)
            keys = [c.key(s) for s in KEY_SIZES]
            for n, size in enumerate([tile - 1, tile, tile + 1, 2 * tile + 5, 17]):
                for mode in (aes_ref.GCM, aes_ref.CTR):
                    c.add(mode, keys[n % 3], size, OFFSETS[n % 5], OFFSETS[(n + 3) % 5], AAD_LENGTHS[n % 7])
            codes, st, out = c.run(decoder)
            assert st.code == abi.OK and not codes.any(), tile
            c.check_output(out)
        for bad in (0, 512, 1536, 65536, -1024):
            with pytest.raises(native.PqgError):
                decoder.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, bad)
    finally:
        decoder.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, abi.AES_TILE_BYTES)


def test_two_thousand_one_block_modules(small_tiles):
    """Many small jobs are the normal case: about 2,000 one-block modules (1 to 16 bytes) in one call, both modes,
    three keys, all offsets."""
    c = Call(3)
    keys = [c.key(s) for s in KEY_SIZES]
    for j in range(2000):
        c.add(aes_ref.GCM if j % 3 else aes_ref.CTR, keys[j % 3], 1 + j % 16, OFFSETS[j % 5], OFFSETS[(j // 5) % 5],
              AAD_LENGTHS[j % 7])
    codes, st, out = c.run(small_tiles)
    assert st.code == abi.OK and not codes.any()
    c.check_output(out)


def _flip(module, byte, bit=0x10):
    return module[:byte] + bytes([module[byte] ^ bit]) + module[byte + 1:]


def _tampered(mode, seed):
    """One call of untouched jobs and tampered ones. -> (call, the tampered jobs' indices)"""
    c = Call(seed)
    k0, k1 = c.key(16), c.key(32)
    n = 3 * T + 40                                  # blocks: first, middle, last (short)
    bad = []
    c.add(mode, k0, n, 1, 3)
    for at in (16, 16 + n // 2, 16 + n - 1):        # the first, a middle, the last ciphertext block
        plain, nonce, aad = c.rng.bytes(n), c.rng.bytes(12), c.rng.bytes(15)
        m = aes_ref.encrypt_module(c.keys[k0], mode, nonce, plain, aad, backend=LIB)
        bad.append(c.add_module(mode, k0, _flip(m, at), plain, aad, 3, 8))
        c.add(mode, k1, 33, 8, 15)
    plain, nonce, aad = c.rng.bytes(100), c.rng.bytes(12), c.rng.bytes(15)
    m = aes_ref.encrypt_module(c.keys[k1], mode, nonce, plain, aad, backend=LIB)
    if mode == aes_ref.GCM:
        bad.append(c.add_module(mode, k1, _flip(m, len(m) - 1), plain, aad))        # the tag
    bad.append(c.add_module(mode, k1, _flip(m, 4 + 5), plain, aad, 15, 1))         # the nonce
    if mode == aes_ref.GCM:
        bad.append(c.add_module(mode, k1, m, plain, _flip(aad, 14), 0, 1))         # the AAD
    c.add(mode, k0, 2 * T + 5)
    # two pages' modules swapped: the page ordinal in the AAD makes both fail
    aads = [aes_ref.module_aad(b"fileaad!", 2, 0, 1, page) for page in (4, 5)]
    plains = [c.rng.bytes(50), c.rng.bytes(50)]
    mods = [aes_ref.encrypt_module(c.keys[k0], mode, c.rng.bytes(12), p, a, backend=LIB) for p, a in zip(plains, aads)]
    if mode == aes_ref.GCM:
        bad.append(c.add_module(mode, k0, mods[1], plains[1], aads[0]))
        bad.append(c.add_module(mode, k0, mods[0], plains[0], aads[1]))
    # the wrong key
    plain, aad = c.rng.bytes(77), c.rng.bytes(13)
    m = aes_ref.encrypt_module(c.keys[k0], mode, c.rng.bytes(12), plain, aad, backend=LIB)
    bad.append(c.add_module(mode, k1, m, plain, aad, 1, 1))
    c.add(mode, k1, 17, 3, 3)
    return c, bad


def test_tag_failures(small_tiles):
    c, bad = _tampered(aes_ref.GCM, 11)
    assert len(bad) == 9
    codes, st, out = c.run(small_tiles)
    want = np.zeros(len(c.rows), dtype=np.int32)
    want[bad] = abi.ERR_TAG
    assert (codes == want).all(), (codes, want)
    assert st.code == abi.ERR_TAG and st.page == min(bad) and b"GCM tag check failed" in st.message
    c.check_output(out, skip=bad)   # the untouched ones decrypt; nothing leaves any destination range


def test_ctr_verifies_nothing(small_tiles):
    """The same tampering in CTR mode: PQG_OK, and output that differs, as in the reference."""
    c, bad = _tampered(aes_ref.CTR, 12)
    assert len(bad) == 5
    codes, st, out = c.run(small_tiles)
    assert st.code == abi.OK and not codes.any()
    c.check_output(out, skip=bad)
    for j in bad:
        dst, plain = c.want[j]
        assert out[dst:dst + len(plain)].tobytes() != plain
        # ... and it is what AesCtrDecryptor returns for those bytes
        module = dict(c.src)[c.rows[j][0]]
        assert out[dst:dst + len(plain)].tobytes() == aes_ref.decrypt_module(c.keys[c.rows[j][6]], aes_ref.CTR, module)


def test_refusals_and_empty_call(decoder):
    L = native.lib()
    d = torch.zeros(64, dtype=torch.uint8, device=decoder.device)
    status = torch.full((4,), -7, dtype=torch.int32, device=decoder.device)
    torch.cuda.synchronize()
    st = abi.Status()
    keys = decoder._key_table([bytes(range(1, 17))])

    def call(rows, ktab=keys, n_src=64, n_dst=64, ctx=decoder.ctx):
        t = np.array(rows, dtype=abi.DECRYPT_JOB_DTYPE)
        return L.pqg_decrypt_pages(ctx, d.data_ptr(), n_src, d.data_ptr(), n_dst, t.ctypes.data if len(t) else None, len(t),
                                   ktab.ctypes.data, len(ktab), None, 0, status.data_ptr(), C.byref(st))

    assert call([]) == abi.OK                                  # n_jobs == 0 launches nothing
    assert L.pqg_decrypt_sync(decoder.ctx, status.data_ptr(), 0, C.byref(st)) == abi.OK
    assert (status.cpu().numpy() == -7).all()
    assert call([(0, 0, 33, 0, 0, abi.DECRYPT_GCM, 0, 0)], ctx=None) == abi.ERR_INVALID_ARG
    assert call([(0, 0, 33, 0, 0, abi.DECRYPT_GCM, 0, 0), (0, 0, 32, 0, 0, abi.DECRYPT_GCM, 0, 0)]) == abi.ERR_CORRUPT
    assert st.code == abi.ERR_CORRUPT and st.page == 1 and b"Wrong input length" in st.message
    assert call([(0, 0, 16, 0, 0, abi.DECRYPT_CTR, 0, 0)]) == abi.ERR_CORRUPT and st.page == 0
    assert call([(40, 0, 33, 0, 0, abi.DECRYPT_GCM, 0, 0)]) == abi.ERR_INVALID_ARG      # leaves n_src
    assert call([(0, 64, 33, 0, 0, abi.DECRYPT_GCM, 0, 0)]) == abi.ERR_INVALID_ARG      # leaves n_dst
    assert call([(0, 0, 33, 0, 1, abi.DECRYPT_GCM, 0, 0)]) == abi.ERR_INVALID_ARG       # leaves the AAD blob
    assert call([(0, 0, 33, 0, 0, 2, 0, 0)]) == abi.ERR_INVALID_ARG
    assert call([(0, 0, 33, 0, 0, abi.DECRYPT_GCM, 1, 0)]) == abi.ERR_INVALID_ARG
    assert call([(0, 0, 33, 0, 0, abi.DECRYPT_GCM, 0, 1)]) == abi.ERR_INVALID_ARG
    for bad_key in (bytes(16), bytes(32), b"x" * 15, b"x" * 17):
        assert call([(0, 0, 33, 0, 0, abi.DECRYPT_GCM, 0, 0)], ktab=decoder._key_table([bad_key])) == abi.ERR_INVALID_ARG
    assert (status.cpu().numpy() == -7).all()                  # nothing was launched


def test_copy_ranges(decoder):
    """pqg_copy_ranges: ranges of every length up to a few waves at all offsets; a range that leaves either buffer is
    skipped; nothing else in the destination changes."""
    rng = np.random.default_rng(31)
    src = rng.integers(0, 256, size=20000, dtype=np.uint8)
    rows, want, pos, dpos = [], np.full(30000, CANARY, dtype=np.uint8), 0, 7
    for n in list(range(0, 70)) + [127, 128, 129, 300]:
        rows.append((pos, dpos, n, 0))
        want[dpos:dpos + n] = src[pos:pos + n]
        pos, dpos = pos + n + n % 3, dpos + n + 1 + n % 5
    rows += [(19990, 100, 11, 0), (0, 29995, 6, 0), (0, 200, 4, 1), (2**40, 0, 1, 0)]  # skipped
    table = np.array(rows, dtype=abi.COPY_RANGE_DTYPE)
    d_src, d_dst = torch.from_numpy(src).to(decoder.device), torch.from_numpy(np.full(30000, CANARY, dtype=np.uint8)).to(decoder.device)
    d_tab = torch.from_numpy(table.view(np.uint8).copy()).to(decoder.device)
    torch.cuda.synchronize()
    L = native.lib()
    assert L.pqg_copy_ranges(decoder.ctx, d_src.data_ptr(), 20000, d_dst.data_ptr(), 30000, d_tab.data_ptr(), len(rows)) == abi.OK
    assert L.pqg_copy_ranges(decoder.ctx, d_src.data_ptr(), 20000, d_dst.data_ptr(), 30000, None, 0) == abi.OK
    decoder.stream.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
