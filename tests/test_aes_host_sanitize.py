"""The host half of pqg_decrypt_pages under AddressSanitizer + UndefinedBehaviorSanitizer (host only, no HIP):
tests/c/aes_host_main.cpp, a stand-alone program built from csrc/pqgpu_aes_host.cpp with
-fsanitize=address,undefined -fno-sanitize-recover=all, drives the validation, the tile / job / AAD table builder,
the key material (schedule, powers of H, the 4-bit table) and pqg_module_aad with exactly-sized heap buffers:
modules ending at n_src and one byte past it, AADs ending at the blob's end, plaintext sizes around tile
multiples, every key size, output capacities of exactly the AAD's length."""
import os
import subprocess

from test_aes_host import build


def test_aes_host_code_under_asan_ubsan(tmp_path):
    exe = build(str(tmp_path / "aes_host_main"), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                  "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "selfcheck"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.splitlines()[-1].endswith("fail=0")
    key = subprocess.run([exe, "key", "000102030405060708090a0b0c0d0e0f1011121314151617", "32768"], capture_output=True,
                         text=True, env=env, timeout=600)
    assert key.returncode == 0 and key.stdout.count("\npw ") == 2049, key.stderr[-4000:]
