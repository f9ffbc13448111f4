"""tools/run_file.py --snapshot S --antenna FILE ... --array-search: the argument
rules, without a GPU.  (The run itself: tests/test_gpu_snapshot_array.py.)"""
from test_run_file_signature import files, snap  # noqa: F401  (the fixture of empty files)
from test_run_file_spoof import run_file


def test_array_search_rules(files):  # noqa: F811
    (a0, a1, a2), eph = files
    r = run_file(a0, '--antenna', a1, '--null', '--array-search')
    assert r.returncode == 2 and '--array-search needs --snapshot' in r.stderr
    for extra in ([], ['--antenna', a1] * 4, ['--antenna', a1, '--spoof-check'], ['--antenna', a1, '--cancel'],
                  ['--antenna', a1, '--collective', '--near', '49.0,8.0'],
                  ['--antenna', a1, '--spoof-check', '--beams']):
        r = run_file(a0, *snap(eph), '--array-search', *extra)
        assert r.returncode == 2 and '--array-search: with one to three --antenna FILE' in r.stderr, r.stderr[-500:]
    for extra, word in ((['--null'], '--null'), (['--excise'], '--excise'), (['--format', 'sc16'], 'own format')):
        r = run_file(a0, *snap(eph), '--antenna', a1, '--array-search', *extra)
        assert r.returncode == 2 and word in r.stderr
    # legal: the call gets as far as reading the (empty) files
    r = run_file(a0, *snap(eph), '--antenna', a1, '--antenna', a2, '--array-search')
    assert r.returncode != 2 and 'the recording holds 0 samples' in r.stderr, r.stderr[-500:]
