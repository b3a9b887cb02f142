"""DevMem (relearn_amd/csrc/dev_mem.hpp), the owner of every handle's device memory, as a plain C++ program over malloc
(tests/cpp/dev_mem_demo.cpp defines the four allocator functions itself): built with -fsanitize=address,undefined and run
directly, leak checking on.  The program exits non-zero unless the destructor frees everything, `ensure` grows only,
a throwing `ensure` leaves a null pointer that the next call fills, a create that fails on its first, a middle or its
last allocation leaves nothing behind, `release` frees once, a moved-from owner frees nothing and views are ignored."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the compile line of the stand-alone programs of tests/test_sanitizers_cpu.py
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_dev_mem_under_asan_and_ubsan():
    exe = os.path.join(tempfile.mkdtemp(prefix="relearn_devmem_"), "dev_mem_demo")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", ROOT, "-I",
                           os.path.join(ROOT, "include")] + SAN +
                          [os.path.join(ROOT, "tests", "cpp", "dev_mem_demo.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([exe], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = proc.stdout.decode()
    assert proc.returncode == 0, out[-4000:]
    assert "dev_mem ok" in out
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]


def test_dev_mem_header_needs_no_hip():
    """the header is plain C++17: it compiles alone, without a HIP include path"""
    src = '#include "relearn_amd/csrc/dev_mem.hpp"\nint main() { DevMem m; (void)m; return 0; }\n'
    with tempfile.NamedTemporaryFile("w", suffix=".cpp", delete=False) as f:
        f.write(src)
    try:
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-fsyntax-only", f.name])
    finally:
        os.unlink(f.name)
