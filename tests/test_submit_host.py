"""The submission queue of gpsmi_trk_process_stream (csrc/gpsmi_submit.h) under ThreadSanitizer and
under AddressSanitizer + UBSan, without a GPU: tests/host/submit_check.cpp is a program of its own
with a stub step, built here with the host compiler into a temporary directory and run as a child
process.  Nothing is loaded into Python and nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'submit_check.cpp')
INC = os.path.join(ROOT, 'gps-sdr-receiver_amd', 'csrc')
PROBE = 'int main() { return 0; }\n'
# the runtime goes INTO the program (clang++ does so by itself): a program that finds its sanitizer
# as a shared library refuses to start wherever something else is preloaded in front of it
STATIC = {'g++': {'thread': ['-static-libtsan'], 'address,undefined': ['-static-libasan', '-static-libubsan']}}


def _build(tmp, sanitize):
    """-> (path of the binary, None) or (None, why not)."""
    probe = os.path.join(tmp, 'probe.cpp')
    with open(probe, 'w') as f:
        f.write(PROBE)
    why = 'neither g++ nor clang++ found'
    for cxx in ('g++', 'clang++'):
        if not shutil.which(cxx):
            continue
        flags = [cxx, '-std=c++17', '-O1', '-g', '-pthread', '-fno-omit-frame-pointer', f'-fsanitize={sanitize}']
        flags += STATIC.get(cxx, {}).get(sanitize, [])
        r = subprocess.run(flags + [probe, '-o', os.path.join(tmp, 'probe')], capture_output=True, text=True, timeout=120)
        if r.returncode:                # (no runtime to link: the next compiler may have one)
            why = f'{cxx} does not link -fsanitize={sanitize}: {r.stderr.strip()[-200:]}'
            continue
        exe = os.path.join(tmp, 'submit_check')
        r = subprocess.run(flags + ['-Wall', '-Wextra', '-Werror', '-I', INC, SRC, '-o', exe],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f'{cxx} -fsanitize={sanitize}:\n{r.stderr}'
        return exe, None
    return None, why


@pytest.mark.parametrize('sanitize', ['thread', 'address,undefined'])
def test_submit_queue_under_sanitizer(tmp_path, sanitize):
    exe, why = _build(str(tmp_path), sanitize)
    if exe is None:
        pytest.skip(why)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    for word in ('ThreadSanitizer', 'AddressSanitizer', 'runtime error'):
        assert word not in r.stdout, r.stdout[-4000:]
    assert 'submit_check ok' in r.stdout
