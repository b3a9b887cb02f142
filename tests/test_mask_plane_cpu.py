"""relearn_amd/csrc/mask_plane.hpp on the host (tests/cpp/mask_plane_demo.cpp): the layout of the relu' masks a keeping
gradient pass of the fused 5-128-2 policy kernel leaves for the Fisher-vector passes of the same call.  For
all 64 lanes and all 32 pairs, encode then decode returns each of the four values of a pair, on an all-zero and on an
all-one background; pair q owns bit q & 15 and bit 16 + (q & 15) of word q >> 4 and no two pairs share a bit; the decode
of a position is exactly 0x3F80 / 0x3F800000 / their sum / 0; and the encode goes through all 2^16 patterns of each
word's low halves.  Host-only code: no GPU and no device library needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mask_plane_demo.cpp")


def test_layout_encode_and_decode():
    out = os.path.join(tempfile.mkdtemp(), "mask_plane_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out])
    res = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = res.stdout.decode()
    print(text)
    assert res.returncode == 0 and text.startswith("ok "), text
    # 64 lanes x 32 pairs x 2 backgrounds x 4 values x 32 decodes + 2 x 16 x 4 positions + 2 x 65,536 patterns
    assert int(text.split()[1]) == 64 * 32 * 2 * 4 * 32 + 2 * 16 * 4 + 2 * 65536
