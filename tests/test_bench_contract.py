"""The line bench.py prints (as committed from GPU runs: profiles/r01_k_bench.json, round 1, and profiles/r03zz_bench.json,
round 3) carries every field of the measurement contract, and the rocprofv3 summaries committed beside it agree with it on
the dominant kernel; a bare `python bench.py --gpus N` starts its own ranks."""
import csv
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    b = json.load(open(os.path.join(ROOT, 'profiles', 'r01_k_bench.json')))
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in b, k
    assert b['unit'] == 'frames/s' and b['higher_is_better'] is True and b['scaling'] == 'weak' and b['n_gpus'] == 1
    assert b['vs_baseline'] is None and b['dtype'] == 'f32' and b['data'] == 'synthetic'
    assert 'workload' in b['config'] and 'model' not in b['config']
    assert abs(b['value'] - 252 * 1e3 / b['ms_per_step']) / b['value'] < 1e-3          # frames of one pass / time of one pass
    r = b['roofline']
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] in ('GB/s', 'TFLOP/s')
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and 0 < r['frac'] < 1
    assert r['traffic'] is None or r['traffic'] > 0
    c = b['cpu_baseline']
    assert c['kind'] in ('reference', 'port') and c['cores'] >= 1 and c['value'] > 0 and c['unit'] == 'frames/s' and c['sample']


def test_rocprof_summary_agrees_with_the_bench_line():
    b = json.load(open(os.path.join(ROOT, 'profiles', 'r01_k_bench.json')))
    rows = list(csv.DictReader(open(os.path.join(ROOT, 'profiles', 'r01_k_kernels.csv'))))
    dom = max(rows, key=lambda r: float(r['total_us']))
    assert '40->80' in dom['kernel'] and '40>80' in b['roofline']['kernel']
    # HIP events inside bench.py vs rocprofv3's average for the same kernel (profiled runs clock a few % lower)
    assert abs(float(dom['avg_us']) / 1e3 - b['roofline']['avg_launch_ms']) / b['roofline']['avg_launch_ms'] < 0.08
    t = json.load(open(os.path.join(ROOT, 'profiles', 'r01_k_traffic.json')))
    assert abs(t['hbm_bytes_per_launch'] - b['roofline']['traffic']) / t['hbm_bytes_per_launch'] < 0.01


def _bench(*argv, env=None):
    import subprocess
    import sys
    e = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *argv], env=e, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=300)


def test_bare_invocation_with_several_gpus_starts_its_own_ranks():
    """`python bench.py --gpus N` without a launcher's environment (the driver's command) starts N child ranks that
    find each other on 127.0.0.1; rank 0's JSON line is the only thing on stdout."""
    r = _bench('--gpus', '3', '--launch-check')
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert got['world'] == 3 and got['rank_sum'] == 6 and got['master'].startswith('127.0.0.1:')


def test_a_failing_rank_fails_the_launcher():
    """Without a GPU the ranks of a real run die at torch.cuda.set_device: the launcher must report that, not hang or
    exit 0 (on the GPU box the same command runs the 2-rank rehearsal: tests/test_gpu_parity.py)."""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip('the ranks would run')
    r = _bench('--gpus', '2', '--backend', 'gloo', '--single-device', '--steps', '1', '--warmup', '0')
    assert r.returncode != 0 and 'exited with code' in r.stderr and not r.stdout.strip()


def test_round_3_line_carries_the_counters_and_the_input_kind():
    """Round 3: roofline.mfma_busy / hbm_gbps / algorithmic next to the executed figure, config.input, the host-resident-input
    variant in the default line and as a line of its own (profiles/r03zz_*), and the rocprofv3 summaries they come from."""
    b = json.load(open(os.path.join(ROOT, 'profiles', 'r03zz_bench.json')))
    assert b['verified'] is True and b['config']['input'] == 'hbm_resident' and b['vs_baseline'] is None
    r = b['roofline']
    assert 0.3 < r['mfma_busy']['kernel'] < 1 and r['mfma_busy']['source'].startswith('profiles/')
    assert 0 < r['hbm_gbps']['kernel'] < r['hbm_gbps']['peak'] == 8000.0 and r['hbm_gbps']['whole_cnn'] > 0
    assert abs(r['algorithmic']['achieved'] - r['direct_equivalent']) < 1e-6 and r['algorithmic']['frac'] > r['frac']
    rows = list(csv.DictReader(open(os.path.join(ROOT, 'profiles', 'r03zz_kernels.csv'))))
    assert r['kernel'].startswith('conv2 40>80')
    dom = next(q for q in rows if 'wino<40->80' in q['kernel'])
    # (launches under rocprofv3 ran 9 % longer than under HIP events in the un-profiled run on this box; 3 % in round 2)
    assert abs(float(dom['avg_us']) / 1e3 - r['avg_launch_ms']) / r['avg_launch_ms'] < 0.12
    pm = {q['kernel']: q for q in csv.DictReader(open(os.path.join(ROOT, 'profiles', 'r03zz_pmc.csv')))}
    k = pm['conv3x3_wino<40->80,s1,pool>']
    busy = float(k['SQ_VALU_MFMA_BUSY_CYCLES']) / (float(k['GRBM_GUI_ACTIVE']) / 8 * 1024)
    assert 0.6 < busy < 0.8
    # the two stride-2 blocks as one kernel (the default): matrix-pipe bound, and a quarter of the HBM bytes the two separate
    # kernels moved per launch (profiles/r03z_kernels.csv: 1.99 GB)
    f = pm['conv_s2_fused']
    assert 0.6 < float(f['SQ_VALU_MFMA_BUSY_CYCLES']) / (float(f['GRBM_GUI_ACTIVE']) / 8 * 1024) < 0.8
    fk = next(q for q in rows if q['kernel'] == 'conv_s2_fused')
    assert (2 * float(fk['FETCH_SIZE_KB_per_launch']) + float(fk['WRITE_SIZE_KB_per_launch'])) * 1024 < 0.6e9
    assert any(q['name'].startswith('conv0+1') and 'fused' in q['name'] for q in r['kernels'])
    assert not any(q['name'].startswith('conv1 ') for q in r['kernels'])
    hv = b['host_input_variant']
    h = json.load(open(os.path.join(ROOT, 'profiles', 'r03zz_bench_host.json')))
    assert h['config']['input'] == 'host_u16' and h['verified'] is True and 'PCIe-inclusive' in h['metric']
    assert hv['detections'] > 0 and 0.5 < h['value'] / b['value'] < 1.0 and 0.5 < hv['value'] / b['value'] < 1.0
    for w in ('assoc-c3', 'assoc-c4'):
        for a in ('mcf', 'hungarian'):
            q = json.load(open(os.path.join(ROOT, 'profiles', f'r03zz_bench_{w}_{a}.json')))
            assert q['verified'] is True and q['roofline']['bound'] == 'hbm' and q['config']['association'] == a


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_workloads_c4_and_c5_resolve_to_one_gpu_share_of_the_baseline_configurations():
    """`--workload c4 | c5` (BASELINE configs 4 and 5 by name): 1024x1024 frames, the global flow tracker, per GPU one eighth of
    the configuration's detection frames (132 / 68 input frames) whatever --gpus is; explicit --frames / --size win; the other
    workloads keep their defaults."""
    import argparse
    b = _bench_module()
    def resolve(**kw):
        ns = argparse.Namespace(workload='c3', size=None, frames=None, assoc='hungarian', input='hbm')
        ns.__dict__.update(kw)
        return b.resolve_workload(ns)
    a = resolve(workload='c4')
    assert (a.size, a.frames, a.assoc, a.associates, a.big) == (1024, 132, 'mcf', True, True)
    assert 8 * (a.frames - 4) >= 1020                                   # eight shares cover the configuration's 1 020 detection frames
    a = resolve(workload='c5')
    assert (a.size, a.frames, a.assoc, a.associates, a.big) == (1024, 68, 'mcf', True, True) and 8 * (a.frames - 4) >= 508
    a = resolve(workload='c4', frames=36, size=512)
    assert (a.size, a.frames) == (512, 36)
    a = resolve(workload='c3')
    assert (a.size, a.frames, a.assoc, a.associates, a.big) == (512, 256, 'hungarian', True, False)
    a = resolve(workload='c2')
    assert (a.size, a.frames, a.associates, a.big) == (512, 256, False, False)


def test_committed_counters_are_withheld_when_sources_or_command_differ(tmp_path, monkeypatch):
    """roofline.traffic / hbm_gbps / mfma_busy come from committed rocprofv3 summaries: only from a set whose meta file says it
    measured the present conv kernel sources and the present workload arguments -- otherwise null with the reason."""
    import argparse, shutil, sys
    b = _bench_module()
    sys.path.insert(0, os.path.join(ROOT, 'profiles'))
    import profile_meta
    root = tmp_path / 'repo'
    (root / 'profiles').mkdir(parents=True)
    (root / 'axtrack_amd' / 'csrc').mkdir(parents=True)
    for f in profile_meta.KERNEL_SOURCES:
        shutil.copy(os.path.join(ROOT, f), root / f)
    shutil.copy(os.path.join(ROOT, 'profiles', 'r03zz_kernels.csv'), root / 'profiles' / 't_kernels.csv')
    shutil.copy(os.path.join(ROOT, 'profiles', 'r03zz_pmc.csv'), root / 'profiles' / 't_pmc.csv')
    monkeypatch.setattr(b, 'ROOT', str(root))
    args = argparse.Namespace(workload='c3', assoc='hungarian', arith='f32', input='hbm', size=512, frames=256)
    table = [{'name': 'conv2 40>80 +pool', 'launches': 2, 'ms': 1.0}]
    wino = ('conv2', 'conv4', 'conv5', 'conv7', 'conv8', 'conv10')
    # no meta file: withheld
    got = b.committed_counters(table, 'conv2 40>80 +pool', True, wino, 4.0, args)
    assert got['traffic'] is None and got['mfma_busy'] is None and 'no t_meta.json' in got['counters_withheld'][0]
    def meta(tag, argv, sha=None):
        json.dump({'sources_sha256': sha or profile_meta.sources_sha256(str(root)), 'workload_key': profile_meta.workload_key(argv)},
                  open(root / 'profiles' / f'{tag}_meta.json', 'w'))
    meta('t', ['--cpu-frames', '0']); meta('t_pmc', ['--cpu-frames', '0'])
    got = b.committed_counters(table, 'conv2 40>80 +pool', True, wino, 4.0, args)
    assert got['traffic'] > 0 and 0.3 < got['mfma_busy']['kernel'] < 1 and 'counters_withheld' not in got
    # another command line: withheld
    other = argparse.Namespace(**dict(args.__dict__, assoc='mcf'))
    got = b.committed_counters(table, 'conv2 40>80 +pool', True, wino, 4.0, other)
    assert got['traffic'] is None and got['mfma_busy'] is None and 'collected for' in got['counters_withheld'][0]
    # the kernel sources moved on: withheld
    with open(root / profile_meta.KERNEL_SOURCES[0], 'a') as f:
        f.write('\n// edited\n')
    got = b.committed_counters(table, 'conv2 40>80 +pool', True, wino, 4.0, args)
    assert got['traffic'] is None and 'sources have changed' in got['counters_withheld'][0]


def test_round_4_lines_c4_c5_certificate_steady_state_and_matching_counters():
    """Round 4 (profiles/r04j_bench*.json, counters from the set r04h): the driver's line carries counters only because the set's
    meta file matches its kernel sources and command; the lines of other commands say why theirs are withheld; BASELINE configs 4
    and 5 have lines of their own, verified through the flow certificate over all arcs; every line says what its timed passes
    reuse and what one pass over a fresh timelapse object takes."""
    b = json.load(open(os.path.join(ROOT, 'profiles', 'r04j_bench.json')))
    assert b['verified'] is True and b['n_gpus'] == 1 and b['steps'] == 20 and abs(b['value'] - 252e3 / b['ms_per_step']) / b['value'] < 1e-3
    r = b['roofline']
    assert r['mfma_busy']['source'] == 'profiles/r04h_pmc.csv' and r['hbm_gbps']['source'] == 'profiles/r04h_kernels.csv'
    assert 'counters_withheld' not in r and 0.6 < r['mfma_busy']['kernel'] < 0.8 and 0.6 < r['frac'] < 0.75
    ss = b['config']['steady_state']
    assert ss['fresh_timelapse_pass_ms'] > b['ms_per_step'] and 'identity count' in ss['what'] and 'kept-tile list' in ss['what']
    meta = json.load(open(os.path.join(ROOT, 'profiles', 'r04h_meta.json')))
    assert len(meta['sources_sha256']) == 64 and meta['workload_key']['workload'] == 'c3'
    rows = list(csv.DictReader(open(os.path.join(ROOT, 'profiles', 'r04h_kernels.csv'))))
    dom = next(q for q in rows if 'wino<40->80' in q['kernel'])
    assert abs(float(dom['avg_us']) / 1e3 - r['avg_launch_ms']) / r['avg_launch_ms'] < 0.12
    m = json.load(open(os.path.join(ROOT, 'profiles', 'r04j_bench_mcf.json')))
    assert m['verified'] is True and m['verify']['flow_certificate']['ok'] is True and m['roofline']['mfma_busy'] is None
    assert 'collected for' in m['roofline']['counters_withheld'][0]
    for wl, frames, arcs in (('c4', 128, 1000000), ('c5', 64, 500000)):
        q = json.load(open(os.path.join(ROOT, 'profiles', f'r04j_bench_{wl}.json')))
        assert q['verified'] is True and q['config']['detection_frames_per_gpu'] == frames and q['config']['tiles_per_frame'] == 4
        assert f'BASELINE config {wl[1]}' in q['config']['workload'] and '1 of 8 GPU shares' in q['config']['workload']
        v = q['verify']
        assert v['flow_certificate']['ok'] is True and v['flow_certificate']['arcs'] > arcs and v['arc_rows_vs_oracle']['ok'] is True
        assert v['detections_bit_exact_frames'] == frames and v['cnn_max_rel_err'] < 1e-5
        assert q['cpu_baseline']['kind'] == 'port' and q['cpu_baseline']['value'] > 0 and q['roofline']['bound'] == 'mfma'
        assert abs(q['value'] - frames * 1e3 / q['ms_per_step']) / q['value'] < 1e-3
    assert 'EXTRAPOLATED' in json.load(open(os.path.join(ROOT, 'profiles', 'r04j_bench_c5.json')))['cpu_baseline']['sample']
    two = json.load(open(os.path.join(ROOT, 'profiles', 'r04j_bench_2ranks_c4.json')))
    assert two['n_gpus'] == 2 and two['tracks_identical_on_all_ranks'] is True and two['verify']['flow_certificate']['ok'] is True


class _FakeDetections:
    """What dump_outputs reads of an AxonDetections: _host_dets(), _track_flat, IDed_dets_all."""
    def __init__(self, F=40, cap=64, n_ids=30, seed=3):
        import pandas as pd
        import numpy as np
        rng = np.random.default_rng(seed)
        self.cnt = rng.integers(0, cap, F).astype(np.int32)
        self.conf = rng.random((F, cap), dtype=np.float32)
        self.x, self.y = (rng.integers(0, 512, (F, cap)).astype(np.int32) for _ in range(2))
        self._track_flat = rng.integers(-1, n_ids, int(self.cnt.sum())).astype(np.int32)
        vals = rng.random((n_ids, 3 * F))
        vals[vals < 0.3] = np.nan
        self.IDed_dets_all = pd.DataFrame(vals)

    def _host_dets(self):
        return self.cnt, self.conf, self.x, self.y


def test_dump_outputs_writes_float_arrays_of_what_the_step_returned(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 .npy files holding the detection lists, trajectory ids and IDed_dets_all of the
    last step; past the size limit every array keeps the same seeded sample of rows, and the row indices go beside it."""
    import numpy as np
    b = _bench_module()
    ad = _FakeDetections()
    b.dump_outputs(str(tmp_path / 'all'), ad, True)
    got = {f[:-4]: np.load(tmp_path / 'all' / f) for f in os.listdir(tmp_path / 'all')}
    assert set(got) == {'det_count', 'det_conf', 'det_x', 'det_y', 'track', 'ided_dets_all', 'ided_dets_all_present'}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    valid = np.arange(ad.conf.shape[1])[None, :] < ad.cnt[:, None]
    assert np.array_equal(got['det_count'], ad.cnt) and np.array_equal(got['det_conf'], ad.conf[valid])
    assert np.array_equal(got['det_x'], ad.x[valid]) and np.array_equal(got['det_y'], ad.y[valid])
    assert np.array_equal(got['track'], ad._track_flat)
    ided = ad.IDed_dets_all.to_numpy()
    assert np.isnan(ided).any() and np.array_equal(got['ided_dets_all_present'], ~np.isnan(ided))
    assert np.array_equal(np.where(got['ided_dets_all_present'] == 1, got['ided_dets_all'], np.nan), ided, equal_nan=True)
    b.dump_outputs(str(tmp_path / 'dets'), ad, False)
    assert sorted(os.listdir(tmp_path / 'dets')) == ['det_conf.npy', 'det_count.npy', 'det_x.npy', 'det_y.npy']
    # over the limit: a seeded sample, the same on every call, within the limit
    monkeypatch.setattr(b, 'DUMP_LIMIT_BYTES', 20000)
    for run in ('s1', 's2'):
        b.dump_outputs(str(tmp_path / run), ad, True)
    names = sorted(os.listdir(tmp_path / 's1'))
    assert names == sorted(os.listdir(tmp_path / 's2')) and 'track_rows.npy' in names and 'ided_dets_all_rows.npy' in names
    assert sum(os.path.getsize(tmp_path / 's1' / f) - 128 for f in names) <= 20000
    for f in names:
        a = np.load(tmp_path / 's1' / f)
        assert np.isfinite(a).all() and np.array_equal(a, np.load(tmp_path / 's2' / f)), f
    rows = np.load(tmp_path / 's1' / 'track_rows.npy').astype(np.int64)
    assert np.array_equal(np.load(tmp_path / 's1' / 'det_x_rows.npy'), rows)          # one length, one sample
    assert np.array_equal(np.load(tmp_path / 's1' / 'track.npy'), ad._track_flat[rows])
    ided_rows = np.load(tmp_path / 's1' / 'ided_dets_all_rows.npy').astype(np.int64)
    assert np.array_equal(np.load(tmp_path / 's1' / 'ided_dets_all.npy'), np.nan_to_num(ided[ided_rows], nan=0.0))
    assert np.array_equal(np.load(tmp_path / 's1' / 'ided_dets_all_present_rows.npy'), ided_rows)


def test_full_and_dump_outputs_are_options_of_the_benchmark():
    r = _bench('--help')
    assert r.returncode == 0 and '--full' in r.stdout and '--dump-outputs' in r.stdout
