"""The pre-folded SeaHash helpers of csrc/device_prelude.hpp (what the generated request-group kernel hashes with: the finish's
K2 ^ K3 ^ <bytes> lives inside the memoised tail and the order lane) equal the unfolded forms -- SeaStream, sea_pair, sea_inner3 -- that the
static kernels, the host and the SeaStream emitters keep using.  tests/cpp/sea_fold_host.cpp is a stand-alone HOST program (the prelude's hash
functions are __host__ __device__): 10^6 random inputs + edge values, built with the address and undefined-behaviour sanitizers and run here.
No GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sea_fold_host.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_folded_seahash_helpers_equal_the_unfolded_ones_under_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sea_fold_host")
    deps = [SRC, os.path.join(ROOT, "bevy_ggrs_amd", "csrc", "device_prelude.hpp")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wall",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer",
                               SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sea_fold_host: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
