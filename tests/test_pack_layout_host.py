"""The arithmetic behind the host entries' packed buffers -- where each array of one allocation starts and how large the
allocation is (pangenomix_amd/csrc/pgx_pack.h) -- in a stand-alone C++ program built with AddressSanitizer and UBSan
(tests/pack_layout_check.cpp). No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pack_offsets_match_the_workspace_layout_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler (the build of libpgx needs one too)'
    exe = str(tmp_path / 'pack_layout_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'pack_layout_check.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'pack_layout: ok' in out.stdout
