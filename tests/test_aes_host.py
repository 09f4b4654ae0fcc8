"""The host half of pqg_decrypt_pages alone (csrc/pqgpu_aes_host.cpp, no device): tests/c/aes_host_main.cpp runs
the validation refusals, the tile / job / AAD tables and pqg_module_aad, and prints the key material (the
schedule, the powers of H, the 4-bit table of H^64 applied to sample blocks), which is compared with
tests/aes_ref.py here."""
import os
import subprocess

import pytest

import aes_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "parquet-mr_amd", "csrc")


def build(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "c", "aes_host_main.cpp"), os.path.join(CSRC, "pqgpu_aes_host.cpp"),
                    "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("aes_host") / "aes_host_main"))


def test_validation_and_tables(exe):
    out = subprocess.run([exe, "selfcheck"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:]
    last = out.stdout.splitlines()[-1].split()
    assert last[0] == "selfcheck" and last[2] == "fail=0" and int(last[1].split("=")[1]) > 300


@pytest.mark.parametrize("key_size,tile", [(16, 1024), (24, 1024), (32, 4096)])
def test_key_material_against_aes_ref(exe, key_size, tile):
    key = bytes((7 * i + key_size) & 255 for i in range(key_size))
    out = subprocess.run([exe, "key", key.hex(), str(tile)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert lines[0] == ["rounds", str(key_size // 4 + 6)]
    assert [int(w, 16) for w in lines[1][1:]] == aes_ref.round_key_words(key)
    h = aes_ref.hash_subkey(key)
    pw = {int(ln[1]): int(ln[2], 16) for ln in lines if ln[0] == "pw"}
    xt = {int(ln[1]): int(ln[2], 16) for ln in lines if ln[0] == "xt"}
    assert sorted(pw) == list(range(tile // 16 + 1)) and sorted(xt) == list(range(65))
    p = 1 << 127
    for k in range(tile // 16 + 1):
        assert pw[k] == p, k
        p = aes_ref.gf_mul(p, h)
    hb, p = pw[tile // 16], 1 << 127
    for k in range(65):
        assert xt[k] == p, k
        p = aes_ref.gf_mul(p, hb)
    muls = [ln for ln in lines if ln[0] == "h64mul"]
    assert len(muls) == 4
    for _, x, z in muls:
        assert int(z, 16) == aes_ref.gf_mul(int(x, 16), pw[64])
    block = [ln for ln in lines if ln[0] == "block"][0][1]
    assert block == aes_ref.encrypt_block(aes_ref.expand_key(key), bytes(17 * i for i in range(16))).hex()
