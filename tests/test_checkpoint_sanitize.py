"""The time-window checkpoint codecs (flink_amd/csrc/fw_ckpt_format.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as host code and driven by flink_amd/csrc/ckpt_san_driver.hip: for the
key-group blob and the whole-handle blob of three hand-built states, encode -> decode -> encode is
byte-identical, every proper prefix is refused, and every single-field corruption a damaged savepoint
could carry is refused with the output state untouched.  The program makes no HIP call and needs no
device; any sanitizer report aborts it, so a clean exit is the assertion."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flink_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_checkpoint_codecs_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "san", f"HIPCC={HIPCC}"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(CSRC, "ckpt_san_driver")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    assert [l.split()[0] for l in lines[:-1]] == ["one_word", "hop_block", "key_rows"]
