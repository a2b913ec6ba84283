"""The argument contract of the C ABI, checked without a GPU (tests/contract_cases.py is the table):

  signatures  every prototype of include/*.h against axtrack_amd/_lib.SIGNATURES: return type, argument count and the class
              of every argument (pointer / int / int64_t / size_t / float / double / POINTER(int | int64_t | size_t));
  coverage    every scalar parameter of every declared function has a row, every `free` row quotes the header;
  refusals    every derived out-of-contract call returns AXT_EINVAL before any HIP call, with a message that names the
              function, and leaves every buffer and host output it was handed as it was -- run by tests/contract_child.py in
              a fresh process that cannot see a device (its first line proves that)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import contract_cases as cc
from axtrack_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
# either of these hides the devices from the HIP runtime of the child (CUDA_VISIBLE_DEVICES does not); the child's control decides
HIDDEN = {'HIP_VISIBLE_DEVICES': '-1', 'ROCR_VISIBLE_DEVICES': '-1'}

PROTOS = cc.prototypes()


# ===================================================================================================== signatures
def binding_class(t):
    """Class of a ctypes type of the binding, in the words of contract_cases.classify."""
    if t is None:
        return 'void'
    if t is ctypes.c_void_p:
        return 'pointer'
    if t is ctypes.c_char_p:
        return 'pointer:char'
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        inner = t._type_
        return 'pointer:pointer' if inner is ctypes.c_void_p else 'pointer:' + binding_class(inner)
    names = {ctypes.c_int: 'int', ctypes.c_int32: 'int', ctypes.c_int64: 'int64_t', ctypes.c_longlong: 'int64_t', ctypes.c_long: 'int64_t',
             ctypes.c_size_t: 'size_t', ctypes.c_float: 'float', ctypes.c_double: 'double'}
    for k, v in names.items():              # (c_int64 and c_long are one class on LP64, c_size_t its own: first match in this order)
        if t is k:
            return v
    raise AssertionError(f'the binding uses {t}, which the header classes do not cover')


def compatible(binding, header):
    """A binding class fits a header class: scalars exactly; c_void_p any pointer; POINTER(x) only a pointer to x."""
    if binding == header:
        return True
    if binding == 'pointer':
        return header.startswith('pointer') and header != 'pointer:char'
    return False


def signature_mismatches(signatures, protos=PROTOS):
    out = []
    for name, (ret, params) in protos.items():
        if name not in signatures:
            out.append(f'{name}: no signature')
            continue
        res, args = signatures[name]
        if not compatible(binding_class(res), ret):
            out.append(f'{name}: returns {ret}, the binding says {binding_class(res)}')
        if len(args) != len(params):
            out.append(f'{name}: {len(params)} arguments, the binding has {len(args)}')
            continue
        for k, (t, (pname, pclass, ctype)) in enumerate(zip(args, params)):
            if not compatible(binding_class(t), pclass):
                out.append(f'{name}: argument {k} `{ctype} {pname}` is {pclass}, the binding says {binding_class(t)}')
    return out


def test_signatures_match_the_headers():
    assert len(PROTOS) >= 90
    assert set(PROTOS) == set(_lib.SIGNATURES)
    assert signature_mismatches(_lib.SIGNATURES) == []


def test_signature_check_sees_a_seeded_mismatch():
    def seeded(name, edit):
        sig = {k: (r, list(a)) for k, (r, a) in _lib.SIGNATURES.items()}
        sig[name] = edit(*sig[name])
        found = signature_mismatches(sig)
        assert len(found) == 1 and found[0].startswith(name + ':'), (name, found)
        return found[0]

    def at(k, t):
        return lambda res, args: (res, args[:k] + [t] + args[k + 1:])

    assert 'int64_t' in seeded('axt_render_frames', at(2, ctypes.c_int))                       # int64_t mask_stride as c_int
    assert 'double' in seeded('axt_obs_costs', at(5, ctypes.c_float))                          # double max_conf_cost as c_float
    assert 'float' in seeded('axt_preprocess_u16', at(8, ctypes.c_double))                     # float scale as c_double
    assert 'int64_t' in seeded('axt_hungarian_pairs', at(13, ctypes.c_int))                    # int64_t thr_units
    assert 'pointer' in seeded('axt_tile_occupancy', at(1, ctypes.c_void_p))                   # int T_all as a pointer
    assert 'pointer:int64_t' in seeded('axt_target_field', at(8, ctypes.POINTER(ctypes.c_int64)))      # int *n_rounds as POINTER(c_int64)
    assert 'size_t' in seeded('axt_mot_scores', at(21, ctypes.POINTER(ctypes.c_int)))           # size_t *scratch_bytes as POINTER(c_int)
    assert 'arguments' in seeded('axt_build_arcs', lambda res, args: (res, args[:-1]))         # 28 arguments, 27 bound
    assert 'returns' in seeded('axt_jpeg_scan_bound', lambda res, args: (ctypes.c_int, args))  # int64_t return as c_int
    assert 'returns' in seeded('axt_cnn_flops_per_tile', lambda res, args: (ctypes.c_float, args))


# ===================================================================================================== coverage
def coverage_gaps(protos, rows=cc.ROWS):
    out = []
    for name, proto in protos.items():
        want = [p for p, _ in cc.scalar_params(proto)]
        if name not in rows:
            out.append(f'{name}: no rows at all ({", ".join(want) or "no scalar parameters"})')
            continue
        out += [f'{name}: no row for {p}' for p in want if p not in rows[name]]
        out += [f'{name}: a row for {p}, which is no scalar parameter of it' for p in rows[name] if p not in want]
    out += [f'{name}: rows for a function no header declares' for name in rows if name not in protos]
    return out


def test_every_scalar_parameter_has_a_row():
    assert coverage_gaps(PROTOS) == []
    n_params = sum(len(cc.scalar_params(p)) for p in PROTOS.values())
    assert n_params == sum(len(r) for r in cc.ROWS.values())
    # a new function without rows fails by name
    more = dict(PROTOS, axt_new_entry=('int', [('d_x', 'pointer', 'const int32_t *'), ('n', 'int', 'int'), ('scale', 'double', 'double')]))
    assert coverage_gaps(more) == ['axt_new_entry: no rows at all (n, scale)']
    more['axt_obs_costs'] = ('int', PROTOS['axt_obs_costs'][1] + [('gamma', 'double', 'double')])
    assert 'axt_obs_costs: no row for gamma' in coverage_gaps(more)


def test_every_free_row_quotes_the_header():
    prose = cc.header_prose()
    missing = [f'{fn}.{p}: the headers do not say "{row.sentence}"' for fn, rows in cc.ROWS.items() for p, row in rows.items()
               if isinstance(row, cc.free) and row.sentence not in prose]
    assert missing == []


def test_every_function_is_either_callable_or_names_its_handle():
    for name in PROTOS:
        assert (name in cc.BUILDERS) != (name in cc.HANDLE), f'{name}: needs a builder or the handle it cannot be called without'
    for name, build in cc.BUILDERS.items():
        got = [n for n, _ in build()]
        assert got == [p for p, _, _ in PROTOS[name][1]], f'{name}: the builder\'s arguments are not the header\'s: {got}'
        for (n, v), (_, pclass, _) in zip(build(), PROTOS[name][1]):
            if pclass.startswith('pointer'):
                assert v is None or isinstance(v, (cc.Dev, cc.Host)), f'{name}: {n} is a pointer'
            else:
                assert isinstance(v, float if pclass in ('float', 'double') else int), f'{name}: {n} = {v!r} is no {pclass}'


def test_derived_calls_are_complete():
    """Every refusal and limit builds; ids are unique; every domain with a bound contributes."""
    refusals, limits = cc.refusals(), cc.limits()
    ids = [c.id for c in refusals + limits]
    assert len(set(ids)) == len(ids)
    for c in refusals + limits:
        assert [n for n, _ in c.args] == [p for p, _, _ in PROTOS[c.function][1]], c.id
    for fn in cc.BUILDERS:
        for p, row in cc.ROWS[fn].items():
            if isinstance(row, cc.Dom):
                n_ref = sum(c.function == fn and c.probe == p for c in refusals)
                assert n_ref == (row.below is not None) + (row.above is not None) + (row.kind == 'float') * (2 - row.inf_ok), (fn, p)
                assert row.kind == 'int' or (row.lo is None) == (row.below is None), f'{fn}.{p}: a float bound names its refused neighbour'
    assert len(refusals) >= 300 and len(limits) >= 240


# ===================================================================================================== refusals
# the calls of the issue that the parent commit let through to a HIP call, by the id the table gives them
MUST_REFUSE = [
    'axt_build_arcs[H=0]', 'axt_build_arcs[W=0]', 'axt_build_arcs[max_dist=0]', 'axt_build_arcs[max_dist=32768]',
    'axt_build_arcs[rule 2: 0 <= h_dmax[g] <= 32767: below]',
    'axt_build_arcs[rule 1: n_frames * cap * max_gap <= 2^31 - 1 (computed in size_t)]',
    'axt_build_arcs[rule 4: h_dmax[g] <= max_dist with lengths from d_len_table and d_cost_units]',
    'axt_hungarian_pairs[H=0]', 'axt_hungarian_pairs[max_dist=0]', 'axt_hungarian_pairs[thr_units=-1]',
    'axt_obs_costs[cap=0]', 'axt_obs_costs[max_conf_cost=nan]', 'axt_obs_costs[n_frames=-1]',
    'axt_decode_stitch_nms[rule 2: tile indices 0 .. 32767: below]',
    'axt_decode_stitch_nms[rule 3: tile indices 0 .. 32767: above (40000 would wrap in a short)]',
    'axt_decode_stitch_nms[rule 4: tile indices 0 .. 32767: far above]', 'axt_decode_stitch_nms[conf_thr=nan]',
    'axt_box_histograms[H=0]', 'axt_box_histograms[W=0]', 'axt_box_histograms[box=32769]',
    'axt_tile_occupancy[rule 0: H * W <= 2^31 - 1]', 'axt_track_links[max_gap=256]', 'axt_render_frames[n_out=-1]',
]


@pytest.fixture(scope='module')
def child():
    """The lines of one run of tests/contract_child.py with the devices hidden."""
    env = dict(os.environ, **HIDDEN)
    run = subprocess.run([sys.executable, os.path.join(HERE, 'contract_child.py')], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith('{')]
    print(run.stdout)
    return run, lines


def test_the_child_sees_no_device(child):
    run, lines = child
    assert lines, f'the child printed nothing: {run.stderr[-2000:]}'
    assert lines[0]['device_count'] == 0, f'the child sees {lines[0]["device_count"]} devices: {HIDDEN} does not hide them here'
    begun = [ln['id'] for ln in lines if ln.get('begin')]
    assert run.returncode == 0 and lines[-1].get('done'), (f'the child ended with status {run.returncode} during {begun[-1] if begun else "start-up"}: '
                                                          f'{run.stderr[-2000:]}')


def test_every_refusal_returns_einval_and_touches_nothing(child):
    _, lines = child
    got = {ln['id']: ln for ln in lines if 'rc' in ln and not ln.get('limit')}
    want = cc.refusals()
    assert sorted(got) == sorted(c.id for c in want), 'the child did not make every refusal'
    assert not [i for i in MUST_REFUSE if i not in got], 'a call of the issue is not among the refusals'
    bad = []
    for c in want:
        r = got[c.id]
        if r['rc'] != cc.EINVAL:
            bad.append(f'{c.id}: returned {r["rc"]} ({"reached a HIP call" if r["rc"] == cc.EHIP else "accepted" if r["rc"] == 0 else "?"}): {r["message"]}')
        elif not r['message'] or c.function.replace('_duals', '') not in r['message']:
            bad.append(f'{c.id}: axt_last_error() does not name the function: {r["message"]!r}')
        elif r['touched']:
            bad.append(f'{c.id}: refused, but a buffer or host output it was handed has changed')
    assert not bad, f'{len(bad)} of {len(want)} refusals:\n' + '\n'.join(bad)


def test_no_limit_call_is_refused(child):
    """The limit calls are in the contract: without a device they get past every argument check and fail at the first HIP call
    (AXT_EHIP), or succeed where the work is the host's. (The sentinel regions the child hands out lie 64 KiB apart, so a large
    axt_augment_frames call is refused for overlapping buffers: that refusal is right, and the call runs on the device.)"""
    _, lines = child
    got = {ln['id']: ln for ln in lines if ln.get('limit')}
    assert sorted(got) == sorted(c.id for c in cc.limits())
    bad = [f'{i}: returned {r["rc"]}: {r["message"]}' for i, r in got.items()
           if r['rc'] not in (cc.EHIP, cc.OK, 1) and not (r['rc'] > 0 and 'jpeg' in i) and 'overlaps' not in r['message']]
    assert not bad, '\n'.join(bad)


# ===================================================================================================== host-only limits
HOST_ONLY = ('axt_mcf_solve', 'axt_mcf_solve_duals', 'axt_jpeg_scan_bound', 'axt_jpeg_scratch_bytes')


def test_limits_of_the_host_only_entry_points():
    """The limit calls of the entry points that never touch a device run here too (tests/test_contract_gpu.py runs all)."""
    lib = _lib.load()
    sentinel = cc.sentinel_buffer()
    calls = [c for c in cc.limits() if c.function in HOST_ONLY]
    assert len(calls) >= 14
    for call in calls:
        rc, message, _ = cc.run_refusal(lib, call, sentinel)
        assert rc >= 0, f'{call.id}: returned {rc}: {message}'


def test_flow_certificate_of_an_empty_network():
    """n_det == 0 is in the contract of axt_mcf_solve_duals: no tracks, cost 0, pi(T) = 0 (found by the limit call: the
    potentials of a solver that never ran were read)."""
    lib = _lib.load()
    row_ptr = (ctypes.c_int64 * 1)(0)
    n_tracks, total, pot_t = ctypes.c_int(-9), ctypes.c_int64(-9), ctypes.c_int64(-9)
    for pots in (None, (ctypes.c_int64 * 1)(-9)):
        rc = lib.axt_mcf_solve_duals(0, None, None, None, ctypes.addressof(row_ptr), None, None, 0, 3, None, None, ctypes.byref(n_tracks),
                                     ctypes.byref(total), pots and ctypes.addressof(pots), pots and ctypes.addressof(pots), ctypes.byref(pot_t))
        assert (rc, n_tracks.value, total.value, pot_t.value) == (0, 0, 0, 0)
    assert lib.axt_mcf_solve_duals(0, None, None, None, ctypes.addressof(row_ptr), None, None, 1, 3, None, None, ctypes.byref(n_tracks),
                                   ctypes.byref(total), None, None, ctypes.byref(pot_t)) == 1           # AXT_INFEASIBLE: min_flow 1 of nothing
