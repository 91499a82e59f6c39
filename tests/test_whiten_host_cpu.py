"""
CPU check of the one contract of shg_whiten_rows, shg_whiten_rows_long and shg_whiten_rows_vector (grates_amd/csrc/whiten_host.h): its
rules over accepted, refused and nothing-to-do argument sets of all three calls under a sanitizer (tools/whiten_host_check.cpp, a
stand-alone program).  What the entry points answer through the library is in test_whitening_cpu.py, test_covariance_noise_cpu.py and
test_vector_noise_cpu.py.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rules_run_clean_under_a_sanitizer(tmp_path):
    """the argument rules as a stand-alone CPU program with its own main, built with -fsanitize=address,undefined: nothing of it is
    loaded into Python"""
    compiler = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert compiler, 'a host C++ compiler is needed'
    program = str(tmp_path / 'whiten_host_check')
    subprocess.run([compiler, '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'whiten_host_check.cpp'), '-o', program], check=True)
    done = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and done.stdout.strip() == 'ok', done.stdout
