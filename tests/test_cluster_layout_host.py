"""The host side of the clustering prologue -- run tables of the sorted list from the length histogram and their
expansion to per-sequence lengths and offsets (pangenomix_amd/csrc/cluster_layout.h) -- in a stand-alone C++ program
built with AddressSanitizer and UBSan (tests/cluster_layout_check.cpp). No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_run_tables_and_expansion_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler (the build of libpgx needs one too)'
    exe = str(tmp_path / 'cluster_layout_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'cluster_layout_check.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'cluster_layout: ok' in out.stdout
