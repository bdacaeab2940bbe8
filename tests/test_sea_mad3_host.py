"""The hot path's SeaHash multiply (csrc/device_prelude.hpp sea_mul_p_mad3: x * SEA_P from three 32 x 32 -> 64 products, what the specialised request-group
kernels multiply with) equals x * SEA_P, and the diffuse built on it equals sea_diffuse: the edge values 0, 1, 2^32 - 1, 2^32, 2^64 - 1, either half at
all-ones, every single-bit value and 4096 seeded random values.  tests/cpp/sea_mad3_host.cpp is a stand-alone HOST program built with the address and
undefined-behaviour sanitizers and run here.  No GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sea_mad3_host.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_three_product_multiply_and_hot_diffuse_equal_the_plain_ones_under_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sea_mad3_host")
    deps = [SRC, os.path.join(ROOT, "bevy_ggrs_amd", "csrc", "device_prelude.hpp")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wall",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer",
                               SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sea_mad3_host: ok (16664 comparisons)" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-500:] + r.stderr[-4000:]
