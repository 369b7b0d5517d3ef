"""The host-only logic of a clustering window -- window formation, threshold tables, the in-order walk of a block and the
counting passes (pangenomix_amd/csrc/cluster_resolve.h) -- in a stand-alone C++ program built with AddressSanitizer and
UBSan (tests/cluster_resolve_check.cpp). No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_block_walk_windows_and_thresholds_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler (the build of libpgx needs one too)'
    exe = str(tmp_path / 'cluster_resolve_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'cluster_resolve_check.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'cluster_resolve: ok' in out.stdout
