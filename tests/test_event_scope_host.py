"""The classification of the handles' events (csrc/gpsmi_event_scope.h) on the CPU:
tests/host/event_scope_check.cpp is a program of its own, built here with the host compiler into a
temporary directory and run as a child process.  It asserts that every event the host reads
device-written memory behind is host-visible.  A second check reads the sources: every event
the engines synchronise on or poll from the host is one the classification knows as such."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'event_scope_check.cpp')
INC = os.path.join(ROOT, 'gps-sdr-receiver_amd', 'csrc')


def test_event_classification_is_sound(tmp_path):
    cxx = next((c for c in ('g++', 'clang++') if shutil.which(c)), None)
    if cxx is None:
        pytest.skip('neither g++ nor clang++ found')
    exe = str(tmp_path / 'event_scope_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', INC, SRC, '-o', exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'event_scope_check ok' in r.stdout


# the host-side waits on an event in the engines' sources -> the members they may name
HOST_WAITS = {
    'copied': 'HostVisible', 'in_done': 'HostVisible',        # device-written memory is read behind them
    'ev': 'DeviceOnly', 'corr_stop': 'DeviceOnly',            # stamps alone (gpsmi_trk_wait_prev)
    'staged': 'DeviceOnly',                                   # the host rewrites its own staging arrays
}


def test_every_host_wait_names_a_classified_event():
    """hipEventSynchronize / trk_spin_wait take nothing but the events above, and each of those is
    created with the scope the table gives it.  (hipEventQuery appears in trk_spin_wait alone.)"""
    waits, creates = [], {}
    for name in sorted(os.listdir(INC)):
        text = open(os.path.join(INC, name)).read()
        for m in re.finditer(r'(?:hipEventSynchronize|trk_spin_wait)\(([^;]*)\)\);', text):
            waits.append((name, m.group(1)))
        for m in re.finditer(r'(\w+)(?:\[\w+\])?\.create<Ev::\w+, EventScope::(\w+)>\(\)', text):
            creates.setdefault(m.group(1), set()).add(m.group(2))
        if name != 'gpsmi_trk.hip':
            assert 'hipEventQuery(' not in text, name
    assert len(waits) >= 5
    for name, arg in waits:
        members = set(re.findall(r'(?:->|\.)(\w+)', arg)) - {'timing_pending'}
        members = {m for m in members if m in HOST_WAITS or m in creates}
        assert members and members <= set(HOST_WAITS), (name, arg)
    # (`e` is the loop variable over Slot::ev; corr_stop borrows corr_done or ev[2])
    creates['ev'] = creates.pop('e')
    creates['corr_stop'] = creates['corr_done'] | creates['ev']
    for member, scope in HOST_WAITS.items():
        assert creates[member] == {scope}, member
