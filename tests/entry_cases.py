"""One case per stream-taking entry point of include/axtrack_hip.h, for the convention tests
(tests/test_entry_conventions_cpu.py, tests/test_entry_conventions_gpu.py): "calls are asynchronous on `stream`" and "no
hidden global state: all device state lives in a handle or in caller-provided buffers".

The values these calls compute are judged elsewhere, route by route, against high-precision references (the case modules
next to this file). Here every entry only says how to run the production Python wrapper of one entry point on three
small inputs, and which part of every output the header promises to write:

  real, decoy   two valid inputs of identical shapes and dtypes that give different results in every output: a call that
                reads its input too early (another stream than the caller's) sees the decoy and answers wrongly, never
                out of range -- counts stay within cap, coordinates inside the image, identities below their limits;
  other         a third valid input on the same handle with one scratch-sizing dimension changed (frames, cap, batch);
  call          runs the wrapper(s) on device tensors and returns {name: output}. An output is a device tensor, a host
                array, or a function to call once the stream has been waited for (read-backs, the pinned table);
  promised      per output the elements the header or the wrapper promises to write (default: all), with the sentence
                that says otherwise quoted in `quotes`; `outside` says what the rest must hold afterwards: PATTERN =
                whatever the allocation held (untouched), a number = what the wrapper filled it with, None = nothing
                is promised either way;
  prepare       (optional) the upstream stages of a stage-by-stage call -- track_links before link_paths, the field and
                its samples before target_paths, a trainer's forward before its input_grad. They run on the same kind of
                input as the call, BEFORE the side-stream delay, and hand call() their results; pre_decoy (optional) makes
                a valid decoy of such a result, which then takes part in the side-stream protocol like an input;
  syncs         why the entry point or its wrapper waits for the stream AFTER its own first launches (a count read back, a
                result copied to the host): only the `query` assertion is skipped, the launches up to that wait still
                run behind the delay. None when the call returns with its work still queued;
  waits_first   why the wrapper waits for the stream BEFORE the entry point's first launch (a host array uploaded from
                pageable memory, a device index checked on the host). The delay has run out by then and the real input
                is in place: the side-stream protocol cannot fail for this entry point, which the other protocols still
                cover. The GPU module lists these as NOT_BEHIND_THE_DELAY.

Pure numpy: importable without a GPU. The generators come from the case modules where those have one that can be
reseeded (stagekernel_cases._scatter / _Grid / transition_units, render_cases._small / binned, target_reference's masks,
train_reference.synth_head / synth_table, train_conv_reference.synth_block / synth_inputs); everything else is a seeded
numpy generator here. Shapes are the smallest that still launch every kernel of the call."""
import functools

import numpy as np

PATTERN = 'pattern'
TILE, S, CELLS = 512, 12, 144
KINDS = ('real', 'decoy', 'other')
SEED = {'real': 1, 'decoy': 2, 'other': 3}


class Inputs:
    """dev: {name: array} goes to the device (these are what a stale read would see); host: everything else, passed to
    the wrapper as it is. limits: {name: (lo, hi)} the half-open range the values of that array must lie in to be a valid
    input (count <= cap: (0, cap + 1)); a key (name, column) bounds one column of a table of rows."""

    def __init__(self, dev, host=None, limits=None):
        self.dev = {k: np.ascontiguousarray(v) for k, v in dev.items()}
        self.host = dict(host or {})
        self.limits = dict(limits or {})

    def arrays(self):
        out = dict(self.dev)
        out.update({k: v for k, v in self.host.items() if isinstance(v, np.ndarray)})
        return out


class Entry:
    def __init__(self, name, abi, make, call, handle=None, promised=None, outside=None, quotes=(), syncs=None,
                 fresh_handle=False, prepare=None, pre_decoy=None, waits_first=None):
        self.name, self.abi, self.make, self.call = name, abi, make, call
        self.prepare, self.pre_decoy = prepare, pre_decoy     # see the module docstring; call takes (h, d, p, pre) then
        self.waits_first = waits_first
        self.handle = handle                    # None, 'detector', or a function (host dict of `real`) -> handle
        self.promised = promised                # None or a function (Inputs, {name: array}) -> {name: bool mask}
        self.outside = dict(outside or {})      # {name: PATTERN | number | None}; a name without entry: PATTERN
        self.quotes = tuple(quotes)
        self.syncs = syncs
        self.fresh_handle = fresh_handle        # the call changes the handle by design (a step): every call gets a new one

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def inputs(self, kind):
        return self.make(kind)


ENTRIES = []
# entry points with a `stream` parameter that have no case here: {name: reason}. At most three.
EXCLUDED = {}


def _entry(*a, **k):
    ENTRIES.append(Entry(*a, **k))


def by_abi():
    out = {}
    for e in ENTRIES:
        out.setdefault(e.abi, []).append(e)
    return out


# ================================================================================================== shared generators
def _rng(kind, salt=0):
    return np.random.default_rng(1000 * salt + SEED[kind])


def _frames(rng, T, H, W):
    """f32 frames in [0, 1) with a fifth of the pixels exactly zero."""
    fr = rng.random((T, H, W), dtype=np.float32)
    fr[rng.random((T, H, W)) < 0.2] = 0
    return fr


def _u16(rng, shape):
    """Raw uint16 pixels (stored as the int16 view the wrappers take) around the deployed offset and clip values."""
    return rng.integers(0, 4000, shape).astype(np.uint16).view(np.int16)


def _dets(kind, salt, F, cap, H, W):
    """(conf f32 [F,cap] descending within the count, x, y i32 [F,cap] inside the image, count i32 [F]); the slots beyond
    a count hold in-range values that would make plausible detections (stagekernel_cases._scatter)."""
    import stagekernel_cases as skc
    rng = _rng(kind, salt)
    count = rng.integers(1, cap + 1, F).astype(np.int32)
    count[0] = cap
    count[-1] = cap // 2 - SEED[kind]                # never the same total in two kinds
    x, y = skc._scatter(rng, F, cap, count, H, W)
    conf = np.sort(rng.uniform(0.56, 0.999, (F, cap)).astype(np.float32), axis=1)[:, ::-1]
    return np.ascontiguousarray(conf), x, y, count


def _det_limits(cap, H, W, gcap=None):
    lim = {'x': (0, W), 'y': (0, H), 'count': (0, cap + 1)}
    if gcap is not None:
        lim.update({'gx': (0, W), 'gy': (0, H), 'gcount': (0, gcap + 1)})
    return lim


def _scene(kind, salt, F, n_obj, cap, H, W, p_detect=0.8, jitter=2):
    """Objects on random walks inside the image: labels (gid, gx, gy i32 [F, n_obj], gcount: all present) and detections
    (conf, x, y, count, track i32 [F, cap]) of most of them in shuffled slot order, track = the object's identity, -1 for a
    clutter detection and beyond the count. Identities are unique within a frame on both sides."""
    rng = _rng(kind, salt)
    assert cap >= n_obj + 1
    px = rng.integers(8, W - 8, n_obj).astype(np.int64)
    py = rng.integers(8, H - 8, n_obj).astype(np.int64)
    gid = np.tile(np.arange(n_obj, dtype=np.int32), (F, 1))
    gx, gy = np.zeros((F, n_obj), np.int32), np.zeros((F, n_obj), np.int32)
    x = rng.integers(0, W, (F, cap)).astype(np.int32)
    y = rng.integers(0, H, (F, cap)).astype(np.int32)
    conf = np.sort(rng.uniform(0.56, 0.999, (F, cap)).astype(np.float32), axis=1)[:, ::-1]
    track = np.full((F, cap), -1, np.int32)
    count = np.zeros(F, np.int32)
    for f in range(F):
        px = np.clip(px + rng.integers(-3, 4, n_obj), 3, W - 4)
        py = np.clip(py + rng.integers(-3, 4, n_obj), 3, H - 4)
        gx[f], gy[f] = px, py
        seen = np.nonzero(rng.random(n_obj) < p_detect)[0]
        if f in (0, F - 1):
            seen = np.arange(n_obj)
        slots = rng.permutation(len(seen) + 1)       # one clutter detection per frame
        for s, k in zip(slots[:-1], seen):
            x[f, s] = np.clip(px[k] + rng.integers(-jitter, jitter + 1), 0, W - 1)
            y[f, s] = np.clip(py[k] + rng.integers(-jitter, jitter + 1), 0, H - 1)
            track[f, s] = k
        count[f] = len(seen) + 1
    return dict(conf=np.ascontiguousarray(conf), x=x, y=y, count=count, track=track, gid=gid, gx=gx, gy=gy,
                gcount=np.full(F, n_obj, np.int32))


def _block_mask(rng, H, W, p_on=0.7, block=8):
    """u8 {0, 1} in blocks of 8 x 8 pixels, so that the mask has regions as a corridor mask has."""
    small = (rng.random((-(-H // block), -(-W // block))) < p_on).astype(np.uint8)
    return np.ascontiguousarray(np.kron(small, np.ones((block, block), np.uint8))[:H, :W])


def _serpentine(H, W):
    import target_reference as tgt
    return np.ascontiguousarray(tgt.serpentine_mask(H, W), np.uint8)


def _grid_handle(conn8):
    def make(host):
        from axtrack_amd import hotpath
        return hotpath.Grid(host['mask'], conn8=conn8)
    return make


def _below_count(inp, outs, names, count='count'):
    """Masks of [F, cap, ...] outputs: the slots below each frame's count."""
    cnt = inp.arrays()[count]
    out = {}
    for n in names:
        a = outs[n]
        m = np.arange(a.shape[1])[None, :] < cnt[:, None]
        out[n] = np.broadcast_to(m.reshape(m.shape + (1,) * (a.ndim - 2)), a.shape)
    return out


# ================================================================================================== the detector
IMG = 512


def _cnn_frames(kind, salt, T_real, T_other):
    T = T_other if kind == 'other' else T_real
    return Inputs({'frames': _frames(_rng(kind, salt), T, IMG, IMG)}, {'tile_yx': np.array([[0, 0]], np.int32)})


def _make_cnn_forward(kind):
    B = 3 if kind == 'other' else 1
    return Inputs({'X': _frames(_rng(kind, 10), B * 5, IMG, IMG).reshape(B, 5, IMG, IMG)})


def _call_front_back(det, d, p):
    n = d['frames'].shape[0] - 4
    for t in range(n):                               # one chunk per detection frame, then the back half once
        det.front_frames(d['frames'], p['tile_yx'], t, 1, t)
    return {'yolo': det.back(n, 1)}


_entry('cnn_forward', 'axt_cnn_forward', _make_cnn_forward, lambda det, d, p: {'yolo': det.detect_axons(d['X'])},
       handle='detector')
_entry('cnn_forward_frames', 'axt_cnn_forward_frames', lambda k: _cnn_frames(k, 11, 5, 7),
       lambda det, d, p: {'yolo': det.detect_frames(d['frames'], p['tile_yx'])}, handle='detector')
_entry('cnn_features_frames', 'axt_cnn_features_frames', lambda k: _cnn_frames(k, 12, 5, 7),
       lambda det, d, p: {'feat': det.features_frames(d['frames'], p['tile_yx'])}, handle='detector')
_entry('cnn_block_features_frames', 'axt_cnn_block_features_frames', lambda k: _cnn_frames(k, 13, 5, 7),
       lambda det, d, p: {'feat6': det.features_frames(d['frames'], p['tile_yx'], block=6),
                          'feat4': det.features_frames(d['frames'], p['tile_yx'], block=4)}, handle='detector')
_entry('cnn_front_frames', 'axt_cnn_front_frames', lambda k: _cnn_frames(k, 14, 5, 7), _call_front_back, handle='detector')
_entry('cnn_back', 'axt_cnn_back', lambda k: _cnn_frames(k, 15, 6, 7), _call_front_back, handle='detector')


# ================================================================================================== preprocessing
PREP = dict(offset=121 / 65535, clip_lower=55 / 65535, log_correct=True)


def _make_prep(kind, salt, framewise=False):
    rng = _rng(kind, salt)
    T, H, W = (5 if kind == 'other' else 3), 50, 70
    host = dict(PREP)
    if framewise:
        host['scale'] = rng.uniform(0.01, 0.02, T).astype(np.float32)
    return Inputs({'raw': _u16(rng, (T, H, W)), 'mask': _block_mask(rng, H, W)}, host)


def _call_prep(_, d, p):
    from axtrack_amd import hotpath
    return {'out': hotpath.preprocess_u16(d['raw'], d['mask'], scale=0.015176106, **p)}


def _call_prep_stats(_, d, p):
    from axtrack_amd import hotpath
    st = hotpath.preprocess_stats_u16(d['raw'], d['mask'], **p)
    # the record's `reserved` float is padding: the header gives it no meaning, and it is left out here
    return {k: np.ascontiguousarray(st[k]) for k in ('n', 'sum', 'sumsq', 'max')}


def _call_prep_framewise(_, d, p):
    from axtrack_amd import hotpath
    p = dict(p)
    return {'out': hotpath.preprocess_u16_framewise(d['raw'], p.pop('scale'), d['mask'], **p)}


_entry('preprocess_u16', 'axt_preprocess_u16', lambda k: _make_prep(k, 20), _call_prep)
_entry('preprocess_stats_u16', 'axt_preprocess_stats_u16', lambda k: _make_prep(k, 21), _call_prep_stats,
       syncs='the wrapper returns the statistics as a host array')
_entry('preprocess_u16_framewise', 'axt_preprocess_u16_framewise', lambda k: _make_prep(k, 22, True), _call_prep_framewise,
       waits_first='the wrapper uploads the frame scales from pageable host memory before the launch')


def _make_occupancy(kind):
    rng = _rng(kind, 23)
    T, H, W = (4 if kind == 'other' else 2), 130, 700          # 1 x 2 tiles, the right-hand one 188 px wide
    # nothing but zeros and negative pixels, which do not count, and one pixel > 0: in the left tile (real) or the right one (decoy)
    fr = -rng.random((T, H, W), dtype=np.float32) * (rng.random((T, H, W)) < 0.1)
    x0 = 512 if kind == 'decoy' else 0
    fr[rng.integers(0, T), rng.integers(0, H), x0 + rng.integers(0, 188)] = 0.5
    return Inputs({'frames': fr})


def _call_occupancy(_, d, p):
    from axtrack_amd import hotpath
    return {'occ': hotpath.tile_occupancy_bytes(d['frames'])}


_entry('tile_occupancy', 'axt_tile_occupancy', _make_occupancy, _call_occupancy)


# ================================================================================================== detections
def _make_decode(kind):
    import stagekernel_cases as skc
    rng = _rng(kind, 30)
    F = 5 if kind == 'other' else 3
    keep = [(0, 0), (0, 1)]
    g = skc._Grid(F, keep)
    for f in range(F):
        for k in range(len(keep)):
            cells = rng.choice(CELLS, int(rng.integers(8, 20)) + SEED[kind], replace=False)
            for cell in cells:
                g.put(f, k, int(cell), np.float32(rng.uniform(0.56, 0.99)), keep[k][1] * TILE + int(rng.integers(0, TILE)),
                      keep[k][0] * TILE + int(rng.integers(0, TILE)))
    # every other cell: a confidence below the threshold and offsets inside the cell
    idle = g.yolo[..., 0] == 0
    g.yolo[idle] = np.stack([rng.uniform(0, 0.5, int(idle.sum())), rng.random(int(idle.sum())), rng.random(int(idle.sum()))], 1)
    return Inputs({'yolo': g.yolo}, dict(tile_yx=np.array(keep, np.int32), cap=len(keep) * CELLS + 5))


def _call_decode(_, d, p):
    from axtrack_amd import hotpath
    conf, x, y, count = hotpath.decode_stitch_nms(d['yolo'], p['tile_yx'], cap=p['cap'])
    return dict(conf=conf, x=x, y=y, count=count)


def _promised_decode(inp, outs):
    m = np.arange(outs['x'].shape[1])[None, :] < outs['count'][:, None]
    return {'conf': m, 'x': m, 'y': m}


_entry('decode_stitch_nms', 'axt_decode_stitch_nms', _make_decode, _call_decode, promised=_promised_decode,
       outside=dict(conf=0, x=0, y=0),
       quotes=['hotpath.decode_stitch_nms: "one zeroed block for the four outputs (... slots beyond a frame\'s count stay zero)"'])


def _make_obs(kind):
    F, cap = (6 if kind == 'other' else 4), 200
    conf, _, _, count = _dets(kind, 31, F, cap, 64, 64)
    conf[1, 0] = 40.0 + SEED[kind]                   # the maximum that scale_to_max divides by
    return Inputs(dict(conf=conf, count=count), limits={'count': (0, cap + 1)})


def _call_obs(_, d, p):
    from axtrack_amd import hotpath
    return {'cost': hotpath.obs_costs(d['conf'], d['count'])}


_entry('obs_costs', 'axt_obs_costs', _make_obs, _call_obs, promised=lambda i, o: _below_count(i, o, ['cost']),
       outside=dict(cost=0), quotes=['d_cost f64 [n_frames,cap] (entries >= count are untouched)'])


# ------------------------------------------------------------------------------------------------ masked-grid searches
GH, GW = 60, 130                                     # the grid of every masked case here


def _make_path(kind, salt):
    rng = _rng(kind, salt)
    na, nb = (9 if kind == 'other' else 5), 7
    dev = dict(xa=rng.integers(0, GW, na), ya=rng.integers(0, GH, na), xb=rng.integers(0, GW, nb), yb=rng.integers(0, GH, nb))
    return Inputs({k: v.astype(np.int32) for k, v in dev.items()}, dict(mask=_serpentine(GH, GW), max_dist=100),
                  limits=dict(xa=(0, GW), xb=(0, GW), ya=(0, GH), yb=(0, GH)))


def _call_path_cost(grid, d, p):
    from axtrack_amd import hotpath
    return {'D': hotpath.path_cost(d['xa'], d['ya'], d['xb'], d['yb'], GH, GW, grid, max_dist=p['max_dist'])}


def _call_path_cells(grid, d, p):
    from axtrack_amd import hotpath
    D, cells = hotpath.path_cells(d['xa'], d['ya'], d['xb'], d['yb'], GH, GW, grid, max_dist=p['max_dist'])
    return dict(D=D, cells=cells)


def _promised_path_cells(inp, outs):
    D = outs['D']
    md = inp.host['max_dist']
    return {'cells': (np.arange(md)[None, None, :] < D[:, :, None]) & (D < md)[:, :, None]}


_entry('path_cost', 'axt_path_cost', lambda k: _make_path(k, 32), _call_path_cost, handle=_grid_handle(False))
_entry('path_cells', 'axt_path_cells', lambda k: _make_path(k, 33), _call_path_cells, handle=_grid_handle(False),
       promised=_promised_path_cells, outside=dict(cells=-1),
       quotes=['d_cells i32 [na, nb, max_dist] receives, for every pair with D < max_dist, the D cells of one minimum-cost '
               'path ...; other entries are left untouched'])


def _make_arcs(kind, salt, masked):
    import stagekernel_cases as skc
    F, cap = (8 if kind == 'other' else 6), 12
    H, W = (GH, GW) if masked else (64, 64)
    _, x, y, count = _dets(kind, salt, F, cap, H, W)
    max_dist = 100
    host = dict(shape=(H, W), dmax=np.array([40, 30], np.int32), max_dist=max_dist,
                units=skc.transition_units(2, max_dist) + 1)
    if masked:
        host['mask'] = _serpentine(H, W)
    return Inputs(dict(x=x, y=y, count=count), host, limits=_det_limits(cap, H, W))


def _call_arcs(grid, d, p):
    from axtrack_amd import hotpath
    H, W = p['shape']
    row_ptr, col, length, gap, cost = hotpath.build_arcs(d['x'], d['y'], d['count'], H, W, p['dmax'], p['units'], mask=grid,
                                                         max_dist=p['max_dist'])
    return dict(row_ptr=row_ptr, col=col, length=length, gap=gap, cost=cost)


def _promised_arcs(inp, outs):
    n_det = int(inp.dev['count'].sum())
    return {'row_ptr': np.arange(len(outs['row_ptr'])) <= n_det}


# (row_ptr_kernel writes rows 0 .. n_det and nothing else: the rest of the n_frames*cap+1 the caller allocates is untouched)
_ARCS = dict(promised=_promised_arcs, outside=dict(row_ptr=PATTERN), quotes=['d_row_ptr i64 [n_det+1] (allocate n_frames*cap+1)'],
             syncs='phase 1 reads the number of arcs back')
_entry('build_arcs', 'axt_build_arcs', lambda k: _make_arcs(k, 34, False), _call_arcs, **_ARCS)
_entry('build_arcs[masked]', 'axt_build_arcs', lambda k: _make_arcs(k, 35, True), _call_arcs, handle=_grid_handle(False), **_ARCS)


def _make_hist(kind):
    F, cap, H, W = (5 if kind == 'other' else 3), 10, 130, 200
    _, x, y, count = _dets(kind, 36, F, cap, H, W)
    return Inputs(dict(frames=_frames(_rng(kind, 37), F + 4, H, W), x=x, y=y, count=count), limits=_det_limits(cap, H, W))


def _call_hist(_, d, p):
    from axtrack_amd import hotpath
    hist, hsum = hotpath.box_histograms(d['frames'], d['x'], d['y'], d['count'])
    return dict(hist=hist, hsum=hsum)


_entry('box_histograms', 'axt_box_histograms', _make_hist, _call_hist,
       promised=lambda i, o: _below_count(i, o, ['hist', 'hsum']), outside=dict(hist=0, hsum=0),
       quotes=['axt_box_histograms: "for every detection the 180-bin histogram" -- the slots beyond a count hold no '
               'detection; hotpath.box_histograms hands out zeroed tables'])


# ------------------------------------------------------------------------------------------------ Hungarian association
def _make_hungarian(kind, salt, masked):
    import stagekernel_cases as skc
    F, cap = (7 if kind == 'other' else 5), 16
    s = _scene(kind, salt, F, 10, cap, GH, GW)
    host = dict(dmax=np.array([40, 30], np.int32), max_dist=500, units=skc.transition_units(2, 500))
    if masked:
        host['mask'] = _serpentine(GH, GW)
    return Inputs(dict(x=s['x'], y=s['y'], count=s['count'], units=host.pop('units')), host, limits=_det_limits(cap, GH, GW))


def _call_hungarian(grid, d, p):
    import hungarian_reference as hr
    from axtrack_amd import hotpath
    track, n_tracks = hotpath.hungarian_assoc(d['x'], d['y'], d['count'], GH, GW, p['dmax'], d['units'], hr.THR_UNITS,
                                              max_dist=p['max_dist'], mask=grid)
    return dict(track=track, n_tracks=n_tracks)


_entry('hungarian_pairs', 'axt_hungarian_pairs', lambda k: _make_hungarian(k, 40, True), _call_hungarian,
       handle=_grid_handle(False), syncs='the masked-grid path lengths read the number of open sources back')
_entry('chain_tracks', 'axt_chain_tracks', lambda k: _make_hungarian(k, 41, False), _call_hungarian)


# ------------------------------------------------------------------------------------------------ tables and links
def _make_ided(kind):
    F, cap, n = (8 if kind == 'other' else 6), 12, 10
    s = _scene(kind, 42, F, n, cap, 64, 64)
    return Inputs({k: s[k] for k in ('track', 'conf', 'x', 'y', 'count')}, dict(n_ids=n),
                  limits=dict(track=(-1, n), **_det_limits(cap, 64, 64)))


def _call_ided(_, d, p):
    from axtrack_amd import hotpath
    table, wait = hotpath.ided_table(d['track'], d['conf'], d['x'], d['y'], d['count'], p['n_ids'])

    def read():
        wait()
        return np.array(table)
    return {'table': read}


_entry('ided_table', 'axt_ided_table', _make_ided, _call_ided)


def _make_links(kind, salt, masked):
    F, cap, n = (8 if kind == 'other' else 6), 12, 10
    s = _scene(kind, salt, F, n, cap, GH, GW, p_detect=0.6)
    host = dict(max_gap=3, max_dist=100)
    if masked:
        host['mask'] = _serpentine(GH, GW)
    return Inputs({k: s[k] for k in ('track', 'x', 'y', 'count')}, host, limits=dict(track=(-1, n), **_det_limits(cap, GH, GW)))


def _call_track_links(_, d, p):
    from axtrack_amd import hotpath
    return {'links': hotpath.track_links(d['track'], d['count'], p['max_gap'])}


def _prepare_links(grid, d, p):
    from axtrack_amd import hotpath
    return {'links': hotpath.track_links(d['track'], d['count'], p['max_gap'])}


def _call_link_paths(grid, d, p, pre):
    from axtrack_amd import hotpath
    length, cell_ptr, cells, interp = hotpath.link_paths(pre['links'], d['x'], d['y'], GH, GW, [grid], max_dist=p['max_dist'],
                                                         max_gap=p['max_gap'])
    return dict(length=length, cell_ptr=cell_ptr, cells=cells, interp=interp)


_LINKS_SYNC = 'phase 1 of axt_link_cells reads the number of cells back (after axt_link_paths and its own launch)'
_entry('track_links', 'axt_track_links', lambda k: _make_links(k, 43, False), _call_track_links,
       syncs='the number of links is read back')
_entry('link_paths', 'axt_link_paths', lambda k: _make_links(k, 44, True), _call_link_paths, handle=_grid_handle(False),
       prepare=_prepare_links, syncs=_LINKS_SYNC)
_entry('link_cells', 'axt_link_cells', lambda k: _make_links(k, 45, False), _call_link_paths, prepare=_prepare_links,
       syncs=_LINKS_SYNC)


# ------------------------------------------------------------------------------------------------ target screens
def _target_cells(rng, n):
    return (rng.integers(0, GH, n) * GW + rng.integers(0, GW, n)).astype(np.int32)


def _make_target_field(kind):
    rng = _rng(kind, 50)
    return Inputs({'cells': _target_cells(rng, 5 if kind == 'other' else 3)}, dict(mask=_serpentine(GH, GW)),
                  limits={'cells': (0, GH * GW)})


def _call_target_field(grid, d, p):
    from axtrack_amd import hotpath
    off, moves = hotpath.target_field(d['cells'], GH, GW, grid)
    return dict(off=off, moves=moves)


def _make_target_sample(kind):
    rng = _rng(kind, 51)
    F, cap = (6 if kind == 'other' else 4), 10
    _, x, y, count = _dets(kind, 52, F, cap, GH, GW)
    return Inputs(dict(off=rng.integers(0, 5, (GH, GW)).astype(np.int32), moves=rng.integers(0, 200, (GH, GW)).astype(np.int32),
                       x=x, y=y, count=count), limits=_det_limits(cap, GH, GW))


def _call_target_sample(_, d, p):
    from axtrack_amd import hotpath
    off, moves = hotpath.target_sample(d['off'], d['moves'], d['x'], d['y'], d['count'])
    return dict(det_off=off, det_moves=moves)


def _make_target_paths(kind):
    rng = _rng(kind, 53)
    F, cap = (6 if kind == 'other' else 4), 10
    _, x, y, count = _dets(kind, 54, F, cap, GH, GW)
    return Inputs(dict(cells=_target_cells(rng, 3), x=x, y=y, count=count), dict(mask=_serpentine(GH, GW)),
                  limits=dict(cells=(0, GH * GW), **_det_limits(cap, GH, GW)))


def _prepare_target_paths(grid, d, p):
    from axtrack_amd import hotpath
    off, moves = hotpath.target_field(d['cells'], GH, GW, grid)
    _, det_moves = hotpath.target_sample(off, moves, d['x'], d['y'], d['count'])
    return dict(off=off, moves=moves, det_moves=det_moves)


def _decoy_det_moves(pre):
    # one step more for every detection that has a path: phase 1 would lay out a larger CSR, in which the real paths fit
    m = pre['det_moves']
    return {'det_moves': m + (m >= 0).to(m.dtype)}


def _call_target_paths(grid, d, p, pre):
    from axtrack_amd import hotpath
    cell_ptr, cells = hotpath.target_paths([(pre['off'], pre['moves'])], [grid], d['x'], d['y'], pre['det_moves'], GH, GW)
    return dict(cell_ptr=cell_ptr, cells=cells)


_entry('target_field', 'axt_target_field', _make_target_field, _call_target_field, handle=_grid_handle(False),
       syncs='the host reads the round counter back')
_entry('target_sample', 'axt_target_sample', _make_target_sample, _call_target_sample)
_entry('target_paths', 'axt_target_paths', _make_target_paths, _call_target_paths, handle=_grid_handle(False),
       prepare=_prepare_target_paths, pre_decoy=_decoy_det_moves,
       syncs='phase 1 of axt_target_paths reads the number of cells back (after its own launch)')


# ================================================================================================== mask preparation
def _seg_shape(kind):
    return (70, 100) if kind == 'other' else (96, 130)


def _call_seg_edges(_, d, p):
    from axtrack_amd import hotpath
    P, G, minmax = hotpath.segment_edges(d['img'], sigma=1.0)
    return dict(P=P, G=G, minmax=minmax)


def _call_seg_hist(_, d, p):
    from axtrack_amd import hotpath
    return {'hist': hotpath.segment_histogram(d['G'], 0.0, 1.0)}


def _call_seg_close(_, d, p):
    from axtrack_amd import hotpath
    return {'closed': hotpath.segment_close(d['P'], 0.5, k=4)}


def _make_flood(kind):
    H, W = _seg_shape(kind)
    img = _block_mask(_rng(kind, 63), H, W, p_on=0.6)
    img[H // 2 - 4:H // 2 + 4, :] = 1                # the seed's row band is set: the flood has somewhere to go
    return Inputs({'img': img}, dict(seed=(H // 2, W // 2)))


def _call_seg_flood(_, d, p):
    from axtrack_amd import hotpath
    return {'flooded': hotpath.segment_flood(d['img'], *p['seed'])}


_entry('segment_edges', 'axt_segment_edges', lambda k: Inputs({'img': _u16(_rng(k, 60), _seg_shape(k))}), _call_seg_edges)
_entry('segment_histogram', 'axt_segment_histogram',
       lambda k: Inputs({'G': _rng(k, 61).random(_seg_shape(k), dtype=np.float32)}), _call_seg_hist)
_entry('segment_close', 'axt_segment_close',
       lambda k: Inputs({'P': _rng(k, 62).random(_seg_shape(k), dtype=np.float32)}), _call_seg_close)
_entry('segment_flood', 'axt_segment_flood', _make_flood, _call_seg_flood, syncs='the host reads the round counter back')


# ================================================================================================== metrics
def _make_confusion(kind):
    F, cap, n = (6 if kind == 'other' else 4), 12, 9
    s = _scene(kind, 70, F, n, cap, 130, 200, jitter=12)
    s['gcount'] = np.maximum(s['gcount'] - np.arange(F, dtype=np.int32) % 3, 1)
    return Inputs({k: s[k] for k in ('conf', 'x', 'y', 'count', 'gx', 'gy', 'gcount')},
                  dict(thrs=np.array([0.6, 0.7, 0.8, 0.9])), limits=_det_limits(cap, 130, 200, gcap=n))


def _call_confusion(_, d, p):
    from axtrack_amd import hotpath
    out, fp, fn = hotpath.detection_confusion(d['conf'], d['x'], d['y'], d['count'], d['gx'], d['gy'], d['gcount'], p['thrs'],
                                              k_mask=1)
    return dict(confusion=out, fp_mask=fp, fn_mask=fn)


def _promised_confusion(inp, outs):
    return {**_below_count(inp, outs, ['fp_mask']), **_below_count(inp, outs, ['fn_mask'], 'gcount')}


_entry('detection_confusion', 'axt_detection_confusion', _make_confusion, _call_confusion, promised=_promised_confusion,
       outside=dict(fp_mask=0, fn_mask=0),
       quotes=['d_fp_mask u8 [n_frames, cap] / d_fn_mask u8 [n_frames, gcap]: one byte per detection / label; '
               'hotpath.detection_confusion hands out zeroed masks, the slots beyond a count hold nothing'],
       waits_first='the wrapper uploads the thresholds from pageable host memory before the launch')


def _make_mot(kind):
    F, cap, n = (8 if kind == 'other' else 6), 12, 9
    s = _scene(kind, 71, F, n, cap, 130, 200)
    swapped = s['track'].copy()                      # a second association: two identities trade places half way
    late = swapped[F // 2:]
    a, b = late == 0, late == 1
    late[a], late[b] = 1, 0
    dev = {k: s[k] for k in ('x', 'y', 'count', 'gid', 'gx', 'gy', 'gcount')}
    dev['tracks'] = np.stack([s['track'], swapped])
    # the clutter detection of every frame carries an identity of its own, n: a false positive in its (shuffled) slot
    clutter = (dev['tracks'] < 0) & (np.arange(cap)[None, None, :] < s['count'][None, :, None])
    dev['tracks'][clutter] = n
    return Inputs(dev, dict(no=n, nh=n + 1), limits=dict(tracks=(-1, n + 1), gid=(0, n), **_det_limits(cap, 130, 200, gcap=n)))


def _call_mot(_, d, p):
    from axtrack_amd import hotpath
    names = ('counts', 'tallies', 'ev_kind', 'ev_partner', 'ev_fp')
    return dict(zip(names, hotpath.mot_scores(d['tracks'], d['x'], d['y'], d['count'], d['gid'], d['gx'], d['gy'], d['gcount'],
                                              p['no'], p['nh'], events=True)))


_entry('mot_scores', 'axt_mot_scores', _make_mot, _call_mot)


# ================================================================================================== rendering
def _make_render(kind):
    import render_cases as rc
    from axtrack_amd import render
    ts = (0, 1, 2) if kind == 'other' else (0, 1)
    H, W, sl = 90, 100, (6, 9, 70, 80)
    # the lists of `real`, binned by the production functions; the decoy keeps their shapes and draws other things
    lists_case = rc._small('entry', 114 if kind != 'other' else 115, H, W, sl, (), mask=2, ts=ts, grid=16)
    trail_ptr, trail, prim_ptr, prims = rc.binned(lists_case, render._bin, render._csr)
    trail_col = lists_case.trail_col
    frames, mask = lists_case.frames, lists_case.mask
    if kind == 'decoy':
        other = rc._small('entry_decoy', 116, H, W, sl, (), mask=2, ts=ts, grid=16)
        frames, mask = other.frames, other.mask
        prims = prims.copy()
        glyph = prims[:, 2] == rc.P_GLYPH
        prims[glyph, 3] = (prims[glyph, 3] + 1) % rc.GLYPHS          # the next glyph
        prims[~glyph, 3] += 1                                        # boxes and rectangles one pixel larger
        trail_col = ((trail_col.astype(np.int64) + 7) % 20).astype(np.uint8)
    dev = dict(frames=frames, mask=mask, ts=lists_case.ts, trail_ptr=trail_ptr, trail=trail, trail_col=trail_col,
               prim_ptr=prim_ptr, prims=prims, tables=rc.TABLES)
    # primitive rows (x0, y0, kind, a, b, key, 0, 0): anchors within a tile's width of the output, sizes and glyph codes
    # below the 95 glyphs; trail rows (frame, key, x, y): keys of the colour table, cells within their radius of the output
    Ho, Wo = sl[2:]
    limits = {'ts': (0, len(frames)), 'trail_col': (0, 20), 'tables': (0, 256),
              ('prims', 0): (-64, Wo + 64), ('prims', 1): (-64, Ho + 64), ('prims', 2): (0, 5), ('prims', 3): (0, rc.GLYPHS),
              ('prims', 4): (0, 64), ('prims', 5): (0, 1 << 31), ('prims', 6): (0, 1), ('prims', 7): (0, 1),
              ('trail', 0): (0, len(frames) + 1), ('trail', 1): (1, len(trail_col)), ('trail', 2): (-8, Wo + 8),
              ('trail', 3): (-8, Ho + 8)}
    assert (np.diff(trail_ptr) >= 0).all() and trail_ptr[0] == 0 and trail_ptr[-1] == len(trail)
    assert (np.diff(prim_ptr) >= 0).all() and prim_ptr[0] == 0 and prim_ptr[-1] == len(prims)
    return Inputs(dev, dict(shape=(H, W), slice=sl, grid=16), limits=limits)


def _call_render(_, d, p):
    from axtrack_amd import hotpath
    (H, W), (ymin, xmin, Ho, Wo) = p['shape'], p['slice']
    return {'rgb': hotpath.render_frames(d['frames'], d['mask'], 0, d['ts'], H, W, ymin, xmin, Ho, Wo, p['grid'], True,
                                         d['trail_ptr'], d['trail'], d['trail_col'], d['prim_ptr'], d['prims'], d['tables'])}


_entry('render_frames', 'axt_render_frames', _make_render, _call_render)


# ================================================================================================== fine-tuning
def _make_targets(kind):
    rng = _rng(kind, 80)
    F, cap = (5 if kind == 'other' else 3), 6
    cnt = rng.integers(1, cap + 1, F).astype(np.int32)
    lx = np.full((F, cap), -1, np.int32)
    ly = np.full((F, cap), -1, np.int32)
    for f in range(F):
        lx[f, :cnt[f]] = rng.integers(0, 2 * TILE, cnt[f])
        ly[f, :cnt[f]] = rng.integers(0, TILE, cnt[f])
    return Inputs({}, dict(lx=lx, ly=ly, cnt=cnt, tile_yx=np.array([[0, 0], [0, 1]], np.int32)),
                  limits=dict(lx=(-1, 2 * TILE), ly=(-1, TILE), cnt=(0, cap + 1)))


def _call_targets(_, d, p):
    from axtrack_amd import training
    return {'target': training.yolo_targets((p['lx'], p['ly'], p['cnt']), p['tile_yx'])}


_entry('yolo_targets', 'axt_yolo_targets', _make_targets, _call_targets,
       waits_first='the wrapper uploads the labels from pageable host memory before the launch (the entry has no device '
                   'input of the caller\'s)')

K0, H1, H2 = 24, 8, 8                               # the head of the trainer cases: 24 -> 8 -> 8 -> 432
HEAD_ROWS, HEAD_BATCH = 6, 4
TRAIN_P = dict(LR=1e-3, WEIGHT_DECAY=5e-4)
_INDEX_FIRST = ('the wrapper checks the batch index against the table on the host before the launch (a device index is read '
                'back, a host index uploaded from pageable memory)')


def _head_handle(host):
    import train_reference as tr
    from axtrack_amd import training
    return training.HeadTrainer(dict(zip(training.FC_KEYS, tr.synth_head(K0, H1, H2, 5))), TRAIN_P, max_batch=HEAD_BATCH)


def _make_head(kind, salt):
    import train_reference as tr
    rng = _rng(kind, salt)
    B = 2 if kind == 'other' else HEAD_BATCH
    feats, tgt = tr.synth_table(HEAD_ROWS, K0, 100 * salt + SEED[kind])
    return Inputs(dict(feats=feats, targets=tgt, index=rng.permutation(HEAD_ROWS)[:B].astype(np.int32),
                       yolo=rng.normal(0, 1, (B, S, S, 3)).astype(np.float32), dy=rng.normal(0, 1, (B, S, S, 3)).astype(np.float32)),
                  limits={'index': (0, HEAD_ROWS)})


def _call_head_forward(t, d, p):
    return {'yolo': t.forward(d['feats'], d['index'])}


def _call_head_loss(t, d, p):
    comp, dy = t.loss(d['yolo'], d['targets'], d['index'])
    return dict(components=np.array([comp[k] for k in sorted(comp)]), dy=dy)


def _call_head_step(t, d, p):
    t.forward(d['feats'], d['index'])
    t.step(d['feats'], d['index'], d['dy'])
    out = {f'w{i}': (lambda i=i: t.weights()[i]) for i in range(6)}
    for layer in range(3):
        for j, n in enumerate(('mw', 'vw', 'mb', 'vb')):
            out[f'{n}{layer}'] = (lambda layer=layer, j=j: t.moments(layer)[j])
    return out


def _prepare_head_forward(t, d, p):
    t.forward(d['feats'], d['index'])            # input_grad reads what this forward stashed in the handle
    return {}


def _call_head_input_grad(t, d, p, pre):
    return {'dfeat': t.input_grad(d['dy'])}


_entry('head_trainer_forward', 'axt_head_trainer_forward', lambda k: _make_head(k, 81), _call_head_forward, handle=_head_handle,
       waits_first=_INDEX_FIRST)
_entry('head_trainer_loss', 'axt_head_trainer_loss', lambda k: _make_head(k, 82), _call_head_loss, handle=_head_handle,
       waits_first=_INDEX_FIRST)
_entry('head_trainer_step', 'axt_head_trainer_step', lambda k: _make_head(k, 83), _call_head_step, handle=_head_handle,
       waits_first=_INDEX_FIRST, fresh_handle=True)
_entry('head_trainer_input_grad', 'axt_head_trainer_input_grad', lambda k: _make_head(k, 84), _call_head_input_grad,
       handle=_head_handle, prepare=_prepare_head_forward)

CI, CO, MH, MW = 3, 5, 6, 5                          # the conv block of the trainer cases: 3 -> 5 channels on 6 x 5 maps
CONV_ROWS, CONV_BATCH = 5, 3


def _conv_handle(batch_stats):
    def make(host):
        import train_conv_reference as cr
        from axtrack_amd import training
        sd = {f'blk.{k}': a for k, a in zip(training.CONV_SUFFIXES + training.CONV_STATS, cr.synth_block(CI, CO, 6, scale=2.0))}
        return training.ConvBlockTrainer(sd, 'blk', TRAIN_P, map_size=(MH, MW), max_batch=CONV_BATCH, batch_stats=batch_stats)
    return make


def _make_conv(kind, salt):
    import train_conv_reference as cr
    rng = _rng(kind, salt)
    B = 2 if kind == 'other' else CONV_BATCH
    x, _ = cr.synth_inputs(CONV_ROWS, CI, MH, MW, 100 * salt + SEED[kind])
    return Inputs(dict(x=x, index=rng.permutation(CONV_ROWS)[:B].astype(np.int32),
                       dfeat=rng.normal(0, 1, (B, CO * MH * MW)).astype(np.float32)), limits={'index': (0, CONV_ROWS)})


def _call_conv_forward(t, d, p):
    return {'feat': t.forward(d['x'], d['index'])}


def _call_conv_step(t, d, p):
    t.forward(d['x'], d['index'])
    t.step(d['x'], d['index'], d['dfeat'])
    # With batch statistics "dbias is 0 by definition ..., so conv.bias takes Adam steps of its weight decay alone"
    # (axtrack_hip_stage.h): nothing of the input reaches tensor 1 then, no decoy can change it, and it is left out.
    tensors = [i for i in range(4) if not (t.batch_stats and i == 1)]
    out = {f'w{i}': (lambda i=i: t.weights()[i]) for i in tensors}
    for i in tensors:
        out[f'm{i}'] = (lambda i=i: t.moments(i)[0])
        out[f'v{i}'] = (lambda i=i: t.moments(i)[1])
    if t.batch_stats:
        for k in ('running_mean', 'running_var', 'batch_mean', 'batch_var'):
            out[k] = (lambda k=k: t.stats()[k])
    return out


def _prepare_conv_forward(t, d, p):
    t.forward(d['x'], d['index'])                # input_grad reads the z this forward stashed in the handle
    return {}


def _call_conv_input_grad(t, d, p, pre):
    return {'dx': t.input_grad(d['dfeat'])}


for _bn, _tag in ((False, ''), (True, '[batch_stats]')):
    # (with batch statistics a forward moves the running ones, which none of these outputs but the step's reads)
    _entry('conv_trainer_forward' + _tag, 'axt_conv_trainer_forward', lambda k, s=85 + _bn: _make_conv(k, s), _call_conv_forward,
           handle=_conv_handle(_bn), waits_first=_INDEX_FIRST)
    _entry('conv_trainer_step' + _tag, 'axt_conv_trainer_step', lambda k, s=87 + _bn: _make_conv(k, s), _call_conv_step,
           handle=_conv_handle(_bn), waits_first=_INDEX_FIRST, fresh_handle=True)
    _entry('conv_trainer_input_grad' + _tag, 'axt_conv_trainer_input_grad', lambda k, s=89 + _bn: _make_conv(k, s),
           _call_conv_input_grad, handle=_conv_handle(_bn), prepare=_prepare_conv_forward)


def _make_pool(kind, salt):
    rng = _rng(kind, salt)
    n, H, W = (5 if kind == 'other' else 3), 5, 7
    return Inputs(dict(x=rng.normal(0, 1, (n, H, W)).astype(np.float32),
                       dout=rng.normal(0, 1, (n, H // 2, W // 2)).astype(np.float32)), dict(H=H, W=W))


def _call_pool_forward(_, d, p):
    from axtrack_amd import training
    return {'pooled': training.maxpool2_forward(d['x'], p['H'], p['W'])}


def _call_pool_backward(_, d, p):
    from axtrack_amd import training
    return {'din': training.maxpool2_backward(d['x'], d['dout'], p['H'], p['W'])}


_entry('maxpool2_forward', 'axt_maxpool2_forward', lambda k: _make_pool(k, 91), _call_pool_forward)
_entry('maxpool2_backward', 'axt_maxpool2_backward', lambda k: _make_pool(k, 92), _call_pool_backward)


def _make_augment(kind):
    rng = _rng(kind, 93)
    T, H, W = (5 if kind == 'other' else 3), 70, 600             # 1 x 2 tiles, the right-hand one 88 px wide
    fr = _frames(rng, T, H, W)
    fr[0 if kind == 'decoy' else 1, :, :] = 0                     # one empty frame, another one in the decoy: occupancy differs
    return Inputs({'frames': fr}, dict(transform=dict(dy=3, dx=-5, flip_y=True, flip_x=False, angle=4.0)))


def _call_augment(_, d, p):
    from axtrack_amd import augment
    out, occ = augment.augment_frames(d['frames'], p['transform'], return_occupancy=True)
    return dict(warped=out, occ=occ)


_entry('augment_frames', 'axt_augment_frames', _make_augment, _call_augment)


# ================================================================================================== validity (CPU)
def check_entry(e):
    """What tests/test_entry_conventions_cpu.py demands of every entry's inputs."""
    real, decoy, other = (e.inputs(k) for k in KINDS)
    ra, da, oa = real.arrays(), decoy.arrays(), other.arrays()
    assert set(ra) == set(da) == set(oa), f'{e}: the three inputs name different arrays'
    for k in ra:
        assert ra[k].shape == da[k].shape and ra[k].dtype == da[k].dtype, f'{e}: {k} of real and decoy differ in shape or dtype'
        assert ra[k].dtype == oa[k].dtype, f'{e}: {k} of other has another dtype'
    assert any(ra[k].shape != oa[k].shape for k in ra), f'{e}: `other` has the shapes of `real`'
    assert any(not np.array_equal(ra[k], da[k], equal_nan=ra[k].dtype.kind == 'f') for k in ra), f'{e}: the decoy equals the real input'
    for k in real.host:
        if not isinstance(real.host[k], np.ndarray):
            assert repr(real.host[k]) == repr(decoy.host[k]), f'{e}: host parameter {k} of real and decoy differ'
    for inp in (real, decoy, other):
        arrs = inp.arrays()
        for k, (lo, hi) in inp.limits.items():
            name, col = k if isinstance(k, tuple) else (k, None)           # (name, column): one column of a table of rows
            assert name in arrs, f'{e}: a limit for {name}, which is no array of the input'
            a = arrs[name] if col is None else arrs[name][:, col]
            assert (a >= lo).all() and (a < hi).all(), f'{e}: {k} leaves [{lo}, {hi})'
        for k, a in arrs.items():
            if a.dtype.kind == 'f':
                assert np.isfinite(a).all(), f'{e}: {k} holds a non-finite value'
