"""The argument contract of every function declared in include/*.h, as one table.

ROWS[function][parameter] is, for every SCALAR parameter (int, int32_t, int64_t, size_t, float, double), either

  a domain  I(lo, hi) / F(lo, hi): the accepted range as the header states it. Floating-point domains are finite unless
            `inf_ok` says that an infinity has a meaning; a NaN is always refused.
  free(...) with the header's own sentence (tests/test_contract_cpu.py checks that the header really says it).

RULES[function] holds what a single bound cannot say: a relation between arguments, a product that must fit, the contents
of a host array. From the rows and rules two lists are derived:

  refusals(): complete calls whose other arguments are valid and small and ONE argument lies just outside its domain (or
              is NaN, or makes a product overflow). Each must return AXT_EINVAL before any HIP call
              (tests/test_contract_cpu.py runs them in tests/contract_child.py with the devices hidden).
  limits():   complete, in-contract calls with one argument at the smallest or largest accepted value
              (tests/test_contract_gpu.py runs them on the device).

Both lists exist for the entry points that can be called without a handle (BUILDERS): a builder makes the complete call
from scalar overrides and sizes every buffer from them. Entry points that need a detector, trainer, grid or shard have
their rows here (HANDLE says which handle), so that the coverage rule holds for them; their refusals are tested next to
the code that can make the handle (tests/test_train_*_cpu.py, test_repack_cpu.py, test_cnn_layers_gpu.py).

Pointers get no row: NULL is refused unless the header gives it a meaning, and then it selects a mode of the builder
(grid = NULL, d_len_table, d_hist, d_ctab, d_scratch = NULL: the size query)."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP, OK = -22, -5, 0
INT_MAX = 2 ** 31 - 1
TILE, CELLS = 512, 144
f32, f64, i8, u8, i16, u16, i32, i64 = np.float32, np.float64, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.int64
NAN = float('nan')
FLT_TRUE_MIN = float(np.float32(1e-45))


def cdiv(a, b):
    return -(-a // b)


# ===================================================================================================== the headers
def header_text():
    """All of include/*.h, main header first, the sub-headers in the order it includes them."""
    inc = os.path.join(ROOT, 'include')
    return {fn: open(os.path.join(inc, fn)).read() for fn in sorted(os.listdir(inc)) if fn.endswith('.h')}


def header_prose():
    """The comments of the headers as running text: comment decoration and line breaks collapsed to single blanks."""
    text = '\n'.join(header_text().values())
    text = re.sub(r'^\s*/?\*+/?', ' ', text, flags=re.M)
    return re.sub(r'\s+', ' ', text.replace('*/', ' '))


SCALAR_TYPES = {'int': 'int', 'int32_t': 'int', 'int64_t': 'int64_t', 'size_t': 'size_t', 'float': 'float', 'double': 'double'}


def classify(ctype):
    """Class of a C parameter or return type: 'int', 'int64_t', 'size_t', 'float', 'double', 'void', or for pointers
    'pointer', 'pointer:int' / 'pointer:int64_t' / 'pointer:size_t' (a single pointer to a non-const scalar of that type: what
    a binding may spell POINTER(...)), 'pointer:pointer' and 'pointer:char'."""
    t = re.sub(r'\s+', ' ', ctype.strip())
    if '*' not in t:
        base = t.replace('const ', '').replace('unsigned ', 'unsigned_').strip()
        if base == 'void':
            return 'void'
        if base not in SCALAR_TYPES:
            raise ValueError(f'unknown scalar type {ctype!r}')
        return SCALAR_TYPES[base]
    if t.count('*') >= 2:
        return 'pointer:pointer'
    base = t.replace('*', '').replace('const', '').strip()
    if base == 'char':
        return 'pointer:char'
    if base in ('int', 'int64_t', 'size_t'):
        return 'pointer:' + base
    return 'pointer'


def prototypes():
    """{function: (return class, [(parameter name, class, C type)])} of every prototype in include/*.h, comments stripped."""
    out = {}
    for text in header_text().values():
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        text = re.sub(r'^\s*#.*$', ' ', text, flags=re.M)
        text = re.sub(r'typedef\s+struct\s*\{.*?\}\s*\w+\s*;', ' ', text, flags=re.S)
        text = re.sub(r'typedef\s+struct\s+\w+\s+\w+\s*;', ' ', text)
        text = re.sub(r'extern\s+"C"\s*\{', ' ', text)
        for m in re.finditer(r'([A-Za-z_][\w\s\*]*?)\b(axt_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
            ret, name, args = m.group(1), m.group(2), m.group(3).strip()
            params = []
            if args and args != 'void':
                for a in args.split(','):
                    pm = re.match(r'^(.*?)(\w+)$', a.strip(), flags=re.S)
                    params.append((pm.group(2), classify(pm.group(1)), re.sub(r'\s+', ' ', pm.group(1).strip())))
            assert name not in out, f'{name} is declared twice'
            out[name] = (classify(ret), params)
    return out


def scalar_params(proto):
    return [(n, c) for n, c, _ in proto[1] if not c.startswith('pointer')]


# ===================================================================================================== rows
class Dom:
    """An accepted range [lo, hi] (None = no bound of its own: only the type's range or a rule of RULES limits it).
    below / above: the refused value next to the bound (default lo - 1 / hi + 1 for integers; a float bound must name its own).
    at_lo / at_hi: what else a call needs at (and just beyond) that bound, as overrides of the builder's arguments.
    run_hi + gap: the value the device test runs where the bound itself cannot be allocated or computed in seconds.
    note: the header's wording of the bound, for the reader."""
    kind = 'int'

    def __init__(self, lo=None, hi=None, below=None, above=None, at_lo=None, at_hi=None, beyond_lo=None, beyond_hi=None,
                 run_hi=None, gap=None, inf_ok=False, note=''):
        self.lo, self.hi, self.at_lo, self.at_hi, self.run_hi, self.gap, self.inf_ok, self.note = lo, hi, at_lo or {}, at_hi or {}, run_hi, gap, inf_ok, note
        self.beyond_lo = self.at_lo if beyond_lo is None else beyond_lo
        self.beyond_hi = self.at_hi if beyond_hi is None else beyond_hi
        self.below = below if below is not None else (lo - 1 if lo is not None and self.kind == 'int' else None)
        self.above = above if above is not None else (hi + 1 if hi is not None and self.kind == 'int' else None)
        assert run_hi is None or gap, 'a limit that is not run at its bound states the gap'


class I(Dom):
    kind = 'int'


class F(Dom):
    kind = 'float'


class free:
    """No constraint; `sentence` is the header's own wording (checked against the header)."""

    def __init__(self, sentence):
        self.sentence = sentence


class Rule:
    """What one bound cannot say. refuse: overrides that break the rule (the other arguments valid); limit: overrides of the
    largest accepted combination (None: covered by a row's limit), run only when `run` is true; gap: why not."""

    def __init__(self, text, refuse, limit=None, gap=None, mode=None):
        self.text, self.refuse, self.limit, self.gap, self.mode = text, refuse, limit, gap, mode or {}


# which handle an entry point cannot be called without
HANDLE = {}
ROWS = {}
# the two sentences of the header's conventions that make a parameter free
FLAG = free('Flag arguments (conn8, bg, big_endian, label_quirk, log_correct, flip_y, flip_x, rotate, and `on` of '
            'axt_conv_trainer_set_batch_stats) are read as zero / non-zero: any int is accepted.')
GROUP = free('group (axt_link_paths, axt_target_paths) is any int: a value that no frame carries selects nothing.')
RULES = {}
BUILDERS = {}


class Dev:
    """A device array of a call: `shape` and `dtype`, filled with `fill` or holding `data`; out = the call writes it. Lazy: a
    refusal never allocates it (the child hands a sentinel-filled host array in)."""

    def __init__(self, shape=None, dtype=None, fill=0, data=None, out=False):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype.type
        self.shape, self.dtype, self.fill, self.data, self.out = tuple(int(s) for s in np.atleast_1d(shape)), dtype, fill, data, out

    def array(self):
        return self.data if self.data is not None else np.full(self.shape, self.fill, self.dtype)

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.float64)) * np.dtype(self.dtype).itemsize


class Host:
    """A host array of a call (an h_ pointer, or a host scalar the call writes: n_arcs, scratch_bytes, ...)."""

    def __init__(self, data, out=False, written_on_refusal=False):
        self.data, self.out = np.ascontiguousarray(data), out
        self.written_on_refusal = written_on_refusal         # the header says that a refused call still writes it


def _tiles(n, rows=16):
    """n distinct (row, col) tile indices, row-major on a grid `rows` wide."""
    n = max(int(n), 1)
    return np.array([(k // rows, k % rows) for k in range(min(n, 4096))] + [(0, 0)] * max(n - 4096, 0), i32)


def _lazy(shape):
    return int(np.prod([max(int(s), 0) for s in np.atleast_1d(shape)], dtype=np.float64)) > (1 << 22)


def _in(shape, dtype, make):
    """Input array: made by `make` while small, a lazily filled Dev of zeros beyond (a refusal's shapes may be absurd)."""
    return Dev(shape, dtype) if _lazy(shape) or any(int(s) <= 0 for s in np.atleast_1d(shape)) else Dev(data=np.asarray(make(), dtype))


def _dets(n_frames, cap, H, W, seed, per_frame=5):
    """count i32 [F], x, y i32 [F, cap] as Dev: min(cap, per_frame) detections per frame inside the image."""
    F_ = max(int(n_frames), 0)
    rng = np.random.default_rng(seed)
    xy = lambda lim: _in((F_, cap), i32, lambda: rng.integers(0, max(min(lim, 1 << 20), 1), (F_, max(cap, 0))))
    return Dev((max(F_, 1),), i32, fill=min(max(int(cap), 1), per_frame)), xy(W), xy(H)


def register(name, rows, rules=(), handle=None):
    def deco(builder):
        ROWS[name], RULES[name] = rows, list(rules)
        if handle:
            HANDLE[name] = handle
        else:
            BUILDERS[name] = builder
        return builder
    if handle:
        return deco(None)
    return deco


HW_PRODUCT = 'H * W <= 2^31 - 1'
HW_GAP = 'H * W = 2^31 - 1 needs 2 to 8 GiB per array: run at 2048 x 2048'


def hw_rule(**mode):
    return Rule(HW_PRODUCT, refuse=dict(H=32768, W=65536), limit=dict(H=2048, W=2048), gap=HW_GAP, mode=mode)


# ----------------------------------------------------------------------------------------------------- no arguments
for _n in ('axt_last_error', 'axt_abi_version', 'axt_cnn_flops_per_tile', 'axt_target_tile_size', 'axt_segment_tile_size',
           'axt_render_tile_size', 'axt_augment_frame_chunk'):
    ROWS[_n], RULES[_n] = {}, []
    BUILDERS[_n] = lambda: []

register('axt_cnn_kernel_flops_per_tile', dict(kernel=free('A kernel id outside 0..13 gives 0: there is no error to report.')))(
    lambda kernel=0: [('kernel', kernel)])
register('axt_arc_cost_int', dict(
    cost=free('Pure arithmetic without an error return: any cost, kind, a and b give a value'),
    kind=free('Pure arithmetic without an error return: any cost, kind, a and b give a value'),
    a=free('Pure arithmetic without an error return: any cost, kind, a and b give a value'),
    b=free('Pure arithmetic without an error return: any cost, kind, a and b give a value')))(
    lambda cost=1.0, kind=3, a=1, b=2: [('cost', cost), ('kind', kind), ('a', a), ('b', b)])


# ----------------------------------------------------------------------------------------------------- preprocessing
_PREP_ROWS = dict(
    T=I(1, note='T, H, W >= 1'), H=I(1), W=I(1),
    offset=F(note='offset and clip_lower finite'), clip_lower=F(),
    log_correct=FLAG)


def _prep_raw(T, H, W):
    def make():
        rng = np.random.default_rng(5)
        raw = rng.integers(0, 5000, (T, H, W)).astype(u16)
        raw.reshape(-1)[:3] = (0, 65535, 121)[:raw.size][:3] if raw.size >= 3 else 0
        return raw
    return _in((T, H, W), u16, make)


@register('axt_preprocess_u16', dict(_PREP_ROWS, scale=F(lo=FLT_TRUE_MIN, below=0.0, inf_ok=True, note='scale > 0')), [hw_rule()])
def _preprocess_u16(T=2, H=5, W=9, offset=0.0018, clip_lower=0.0008, log_correct=1, scale=0.015, mask=True):
    return [('d_raw', _prep_raw(T, H, W)), ('d_mask', _in((H, W), u8, lambda: (np.arange(H * W).reshape(H, W) % 5 != 0)) if mask else None),
            ('T', T), ('H', H), ('W', W), ('offset', offset), ('clip_lower', clip_lower), ('log_correct', log_correct), ('scale', scale),
            ('d_out', Dev((T, H, W), f32, out=True)), ('stream', None)]


@register('axt_preprocess_stats_u16', _PREP_ROWS, [
    hw_rule(),
    Rule('*scratch_bytes (in) >= the size the query answers', refuse=dict(scratch=1))])
def _preprocess_stats_u16(T=2, H=5, W=9, offset=0.0018, clip_lower=0.0008, log_correct=1, scratch=None):
    px = max(H, 0) * max(W, 0)
    bpf = max(min((px // 8 + 255) // 256, 2048 // max(T, 1)), 1)
    need = max(T, 1) * bpf * 32
    have = need if scratch is None else scratch
    return [('d_raw', _prep_raw(T, H, W)), ('d_mask', None), ('T', T), ('H', H), ('W', W), ('offset', offset), ('clip_lower', clip_lower),
            ('log_correct', log_correct), ('d_stats', Dev((max(T, 1), 32), u8, out=True)), ('d_scratch', Dev((need,), u8, out=True)),
            ('scratch_bytes', Host(np.array([have], np.uintp), out=True, written_on_refusal=scratch is not None)), ('stream', None)]


@register('axt_preprocess_u16_framewise', _PREP_ROWS, [hw_rule()])
def _preprocess_u16_framewise(T=2, H=5, W=9, offset=0.0018, clip_lower=0.0008, log_correct=1):
    return [('d_raw', _prep_raw(T, H, W)), ('d_mask', None), ('T', T), ('H', H), ('W', W), ('offset', offset), ('clip_lower', clip_lower),
            ('log_correct', log_correct), ('d_scale', Dev((max(T, 1),), f32, fill=0.015)), ('d_out', Dev((T, H, W), f32, out=True)),
            ('stream', None)]


# ----------------------------------------------------------------------------------------------------- tiling, decode
@register('axt_tile_occupancy', dict(
    T_all=I(1, 65539, at_hi=dict(H=3, W=3), note='1 <= T_all <= 65539'), H=I(1), W=I(1)), [hw_rule()])
def _tile_occupancy(T_all=2, H=8, W=8):
    def make():
        fr = np.zeros((T_all, H, W), f32)
        fr[-1, -1, -1] = 1.0                          # one pixel, in the last frame: the scan has to reach it
        return fr
    return [('d_frames', _in((T_all, H, W), f32, make)), ('T_all', T_all), ('H', H), ('W', W),
            ('d_occ', Dev((cdiv(max(H, 1), TILE) * cdiv(max(W, 1), TILE),), u8, out=True, fill=7)), ('stream', None)]


def decode_yolo(n_frames, n_tiles, seed=3, per_frame=12):
    """f32 [F, n_tiles, 12, 12, 3] with `per_frame` cells above 0.55 per frame, two of them close enough to suppress."""
    rng = np.random.default_rng(seed)
    y = np.zeros((n_frames, n_tiles, 12, 12, 3), f32)
    for f in range(n_frames):
        for _ in range(per_frame):
            k, i, j = int(rng.integers(0, n_tiles)), int(rng.integers(0, 12)), int(rng.integers(0, 12))
            y[f, k, i, j] = (rng.uniform(0.56, 0.99), rng.uniform(0, 1), rng.uniform(0, 1))
        y[f, 0, 3, 3] = (0.97, 0.5, 0.5)
        y[f, 0, 3, 4] = (0.60, 0.5, 0.0)               # 21 px below the cell above: dies for min_dist > 21
    return y


@register('axt_decode_stitch_nms', dict(
    n_frames=I(0, note='n_frames == 0: AXT_OK, nothing is touched; negative: AXT_EINVAL'),
    n_tiles=I(1, 256, at_hi=lambda v: dict(cap=v * CELLS), note='1 <= n_tiles <= 256'),
    conf_thr=F(inf_ok=True, note='any number; NaN: AXT_EINVAL'),
    min_dist=I(0, 32767, note='0 <= min_dist <= 32767'),
    cap=I(None, None, note='cap >= n_tiles * 144 (a relation: see the rules)')), [
    Rule('cap >= n_tiles * 144', refuse=dict(n_tiles=2, cap=2 * CELLS - 1), limit=dict(n_tiles=2, cap=2 * CELLS)),
    Rule('n_frames * cap <= 2^31 - 1', refuse=dict(n_frames=1 << 16, cap=1 << 15), limit=dict(n_frames=2, cap=1 << 20),
         gap='n_frames * cap = 2^31 - 1 needs 24 GiB of outputs: run at 2 x 2^20'),
    Rule('tile indices 0 .. 32767: below', refuse=dict(tiles=[(0, 0), (0, -1)])),
    Rule('tile indices 0 .. 32767: above (40000 would wrap in a short)', refuse=dict(tiles=[(0, 0), (40000, 0)])),
    Rule('tile indices 0 .. 32767: far above', refuse=dict(tiles=[(0, 0), (0, 5000000)])),
    Rule('tile indices 0 .. 32767: the largest', refuse=dict(tiles=[(0, 0), (0, 32768)]), limit=dict(tiles=[(0, 0), (32767, 32767)]))])
def _decode_stitch_nms(n_frames=2, n_tiles=2, conf_thr=0.55, min_dist=23, cap=None, tiles=None):
    cap = n_tiles * CELLS if cap is None else cap
    t = _tiles(n_tiles) if tiles is None else np.array(tiles, i32)
    F_ = max(n_frames, 0)
    shape = (F_, n_tiles, 12, 12, 3)
    return [('d_yolo', _in(shape, f32, lambda: decode_yolo(F_, n_tiles))), ('n_frames', n_frames), ('n_tiles', n_tiles),
            ('h_tile_yx', Host(t)), ('conf_thr', conf_thr), ('min_dist', min_dist), ('cap', cap),
            ('d_conf', Dev((F_, cap), f32, out=True)), ('d_x', Dev((F_, cap), i32, out=True)), ('d_y', Dev((F_, cap), i32, out=True)),
            ('d_count', Dev((max(F_, 1),), i32, out=True, fill=-7)), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- association costs
@register('axt_obs_costs', dict(
    n_frames=I(0, note='n_frames == 0: AXT_OK, nothing is touched; negative: AXT_EINVAL'),
    cap=I(1, note='cap >= 1'), method=I(0, 1, note="method 0 = 'scale_to_max', 1 = 'ceil'"),
    max_conf_cost=F(note='max_conf_cost finite')))
def _obs_costs(n_frames=2, cap=8, method=0, max_conf_cost=4.6):
    F_ = max(n_frames, 0)
    count = Dev((max(F_, 1),), i32, fill=min(max(cap, 1), 5))
    conf = lambda: np.random.default_rng(2).uniform(0.56, 1.2, (F_, cap))
    return [('d_conf', _in((F_, cap), f32, conf)), ('d_count', count), ('n_frames', n_frames), ('cap', cap), ('method', method),
            ('max_conf_cost', max_conf_cost), ('d_cost', Dev((F_, cap), f64, out=True)), ('stream', None)]


_PATH_ROWS = dict(
    na=I(0, note='na, nb >= 0'), nb=I(0),
    H=I(1), W=I(1), max_dist=I(1, 32767, at_hi=dict(na=1, nb=2), note='1 <= max_dist <= 32767'),
    conn8=FLAG)


@register('axt_path_cost', _PATH_ROWS, [
    hw_rule(),
    Rule('na * nb <= 2^31 - 1', refuse=dict(na=1 << 16, nb=1 << 15), limit=dict(na=1 << 10, nb=1 << 10),
         gap='na * nb = 2^31 - 1 needs 8 GiB for D: run at 2^10 x 2^10')])
def _path_cost(na=3, nb=4, H=40, W=50, max_dist=30, conn8=0):
    rng = np.random.default_rng(7)
    pts = lambda n, m: _in((max(n, 0),), i32, lambda: rng.integers(0, max(min(m, 1 << 16), 1), max(n, 0)))
    return [('d_xa', pts(na, W)), ('d_ya', pts(na, H)), ('na', na), ('d_xb', pts(nb, W)), ('d_yb', pts(nb, H)), ('nb', nb), ('grid', None),
            ('H', H), ('W', W), ('max_dist', max_dist), ('conn8', conn8), ('d_D', Dev((max(na, 0), max(nb, 0)), i32, out=True, fill=-3)),
            ('stream', None)]


register('axt_path_cells', _PATH_ROWS, [hw_rule()], handle='grid')


_ARC_ROWS = dict(
    n_frames=I(1, note='n_frames >= 1'), cap=I(1, note='cap >= 1'),
    H=I(1, note='H, W >= 1 (not read with d_len_table)'), W=I(1),
    max_dist=I(1, 32767, note='1 <= max_dist <= 32767'),
    conn8=FLAG,
    max_gap=I(1, 8, at_lo=dict(dmax=[9]), at_hi=dict(dmax=[9] * 8, cap=8, n_frames=10), note='1 <= max_gap <= 8'),
    vis_weight=F(lo=float(np.nextafter(0.0, 1.0)), hi=1.0, below=0.0, above=float(np.nextafter(1.0, 2.0)), at_lo=dict(vis=True), at_hi=dict(vis=True),
                 note='vis_weight in (0,1] (read only with d_hist)'),
    miss_rate=F(lo=0.0, below=-0.5, at_lo=dict(vis=True), note='miss_rate finite and >= 0 (read only with d_hist)'),
    edge_cost_thr=F(inf_ok=True, at_lo=dict(vis=True), note='edge_cost_thr any number, NaN refused (read only with d_hist)'))


def _units(max_gap, max_dist):
    n = max(max_dist + 1, 1)
    return np.arange(max(max_gap, 1) * n, dtype=i64).reshape(max(max_gap, 1), n) * 3 + 1000


@register('axt_build_arcs', _ARC_ROWS, [
    hw_rule(),
    Rule('n_frames * cap * max_gap <= 2^31 - 1 (computed in size_t)', refuse=dict(n_frames=70000, cap=70000),
         limit=dict(n_frames=1 << 10, cap=1 << 10, max_gap=2, dmax=[9, 5]), gap='2^31 - 1 slots need 8 GiB of d_work: run at 2^10 x 2^10 x 2'),
    Rule('0 <= h_dmax[g] <= 32767: below', refuse=dict(dmax=[-5, 9])),
    Rule('0 <= h_dmax[g] <= 32767: above', refuse=dict(dmax=[9, 32768]), limit=dict(dmax=[32767, 32767], max_dist=32767)),
    # (stagekernel_cases.length_table_case is the large case at this limit: h_dmax[0] == max_dist, entries == max_dist, units)
    Rule('h_dmax[g] <= max_dist with lengths from d_len_table and d_cost_units', refuse=dict(table=True, max_dist=30, dmax=[31, 9]),
         limit=dict(table=True, max_dist=30, dmax=[30, 30])),
    Rule('h_dmax[g] > max_dist stays accepted on the closed form', refuse=None, limit=dict(max_dist=30, dmax=[40, 35]))])
def _build_arcs(n_frames=4, cap=8, H=64, W=64, max_dist=30, conn8=0, max_gap=2, dmax=None, vis_weight=0.3, miss_rate=0.6,
                edge_cost_thr=0.7, table=False, vis=False, fill=False, units=True, n_arcs=0):
    dmax = np.array([9, 5][:max(max_gap, 1)] if dmax is None else dmax, i32)
    F_, g_ = max(n_frames, 1), max(max_gap, 1)
    count, x, y = _dets(F_, cap, H, W, 21)
    slots = F_ * max(cap, 1)
    work = slots * g_ + F_ + 1 + g_ + 4
    args = [('d_x', x), ('d_y', y), ('d_count', count), ('d_src_count', None),
            ('n_frames', n_frames), ('cap', cap), ('grid', None), ('H', H), ('W', W), ('max_dist', max_dist), ('conn8', conn8),
            ('max_gap', max_gap), ('h_dmax', Host(dmax)),
            ('d_hist', Dev((F_, cap, 180), f32, fill=1.0 / 180) if vis else None), ('d_hist_sum', Dev((F_, cap), f64, fill=1.0) if vis else None),
            ('vis_weight', vis_weight), ('miss_rate', miss_rate), ('edge_cost_thr', edge_cost_thr),
            ('d_row_ptr', Dev((slots + 1,), i64, out=True)), ('d_work', Dev((work,), i32, out=True)),
            ('d_col', Dev((max(n_arcs, 1),), i32, out=True) if fill else None), ('d_len', Dev((max(n_arcs, 1),), i16, out=True) if fill else None),
            ('d_gap', Dev((max(n_arcs, 1),), u8, out=True) if fill else None),
            ('d_cost_units', Dev(data=_units(g_, max_dist)) if units and not _lazy((g_, max_dist)) else None),
            ('d_cost', Dev((max(n_arcs, 1),), i64, out=True) if fill and units else None),
            ('n_arcs', Host(np.array([n_arcs if fill else -77], i64), out=True)),
            ('d_len_table', _in((F_, cap, g_, cap), i16, lambda: length_table(F_, cap, g_, max_dist)) if table else None), ('stream', None)]
    return args


def length_table(F_, cap, g_, max_dist):
    """i16 [F, cap, max_gap, cap]: lengths 1 .. max_dist with max_dist itself among them, some <= 0 (no path)."""
    rng = np.random.default_rng(31)
    tab = rng.integers(-2, max_dist + 1, (F_, cap, g_, cap)).astype(i16)
    tab[:, 0, :, 0] = max_dist
    return tab


@register('axt_box_histograms', dict(
    T_all=I(1, at_lo=dict(t_offset=0, n_frames=1), note='T_all >= 1'), H=I(1), W=I(1),
    t_offset=I(0, note='t_offset >= 0 and t_offset + n_frames <= T_all'),
    n_frames=I(1, 65535, at_hi=lambda v: dict(T_all=v, t_offset=0, H=2, W=2, cap=1, box=2), note='1 <= n_frames <= 65535'),
    cap=I(1, note='cap >= 1'), box=I(1, 32768, note='1 <= box <= 32768')), [
    hw_rule(),
    Rule('t_offset + n_frames <= T_all', refuse=dict(T_all=4, t_offset=3, n_frames=2), limit=dict(T_all=4, t_offset=2, n_frames=2))])
def _box_histograms(T_all=3, H=40, W=50, t_offset=1, n_frames=2, cap=4, box=9):
    count, x, y = _dets(n_frames, cap, H, W, 9, per_frame=3)
    fr = lambda: np.random.default_rng(4).uniform(0, 1, (T_all, H, W))
    F_ = max(n_frames, 0)
    return [('d_frames', _in((T_all, H, W), f32, fr)), ('T_all', T_all), ('H', H), ('W', W), ('t_offset', t_offset),
            ('d_x', x), ('d_y', y), ('d_count', count),
            ('n_frames', n_frames), ('cap', cap), ('box', box), ('d_hist', Dev((F_, cap, 180), f32, out=True)),
            ('d_hist_sum', Dev((F_, cap), f64, out=True)), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- the flow solver (host)
def _network():
    """Three detections in three frames, arcs 0 -> 1, 0 -> 2, 1 -> 2."""
    return (np.array([-5, -5, -5], i64) << 16, np.array([2, 2, 2], i64) << 16, np.array([2, 2, 2], i64) << 16,
            np.array([0, 2, 3, 3], i64), np.array([1, 2, 2], i32), np.array([1, 3, 1], i64) << 16)


_MCF_ROWS = dict(n_det=I(0, at_lo=dict(empty=True), note='n_det >= 0'), min_flow=I(0, note='0 <= min_flow <= max_flow'),
                 max_flow=I(None, None, note='max_flow >= min_flow (a relation)'))
_MCF_RULES = [Rule('min_flow <= max_flow', refuse=dict(min_flow=3, max_flow=2), limit=dict(min_flow=1, max_flow=1))]


def _mcf_args(n_det, min_flow, max_flow, empty):
    obs, en, ex, rp, col, cost = _network()
    if empty:
        rp = np.zeros(1, i64)
    return [('n_det', n_det), ('h_obs', Host(obs)), ('h_entry', Host(en)), ('h_exit', Host(ex)), ('h_row_ptr', Host(rp)), ('h_col', Host(col)),
            ('h_cost', Host(cost)), ('min_flow', min_flow), ('max_flow', max_flow), ('h_next', Host(np.full(3, -9, i32), out=True)),
            ('h_track', Host(np.full(3, -9, i32), out=True)), ('n_tracks', Host(np.array([-9], i32), out=True)),
            ('total_cost', Host(np.array([-9], i64), out=True))]


@register('axt_mcf_solve', _MCF_ROWS, _MCF_RULES)
def _mcf_solve(n_det=3, min_flow=0, max_flow=3, empty=False):
    return _mcf_args(n_det, min_flow, max_flow, empty)


@register('axt_mcf_solve_duals', _MCF_ROWS, _MCF_RULES)
def _mcf_solve_duals(n_det=3, min_flow=0, max_flow=3, empty=False):
    return _mcf_args(n_det, min_flow, max_flow, empty) + [('h_pot_u', Host(np.full(3, -9, i64), out=True)),
                                                           ('h_pot_v', Host(np.full(3, -9, i64), out=True)),
                                                           ('pot_t', Host(np.array([-9], i64), out=True))]


register('axt_mcf_shard_begin', dict(n_det=I(0), rank=I(0, note='0 <= rank < world'), world=I(1, note='world a power of two')),
         handle='shard (made by this call; its refusals stand in tests/test_mcf_shard.py)')
register('axt_mcf_shard_finish', dict(min_flow=I(0), max_flow=I(None, None, note='max_flow >= min_flow')), handle='shard')
register('axt_mcf_shard_finish_duals', dict(min_flow=I(0), max_flow=I(None, None, note='max_flow >= min_flow')), handle='shard')
for _n in ('axt_mcf_shard_export', 'axt_mcf_shard_free'):
    register(_n, {}, handle='shard')


# ----------------------------------------------------------------------------------------------------- Hungarian association
def hungarian_lds(cap, max_dist):
    """hungarian.hip: the bytes of LDS axt_hungarian_pairs needs before the cost cache (lds_base)."""
    return cap * (3 * 8 + 8 * 4 + 2) + 8 + (max_dist + 2) * 8 + 8 + cap * 8 + (cap * 48 if cap <= 576 else 0)


HUNG_LDS = 160 * 1024
HUNG_MAX_DIST_CAP8 = (HUNG_LDS - hungarian_lds(8, 0)) // 8          # the largest max_dist that fits next to cap = 8


@register('axt_hungarian_pairs', dict(
    n_frames=I(1, note='n_frames >= 1'), cap=I(1, 2048, at_hi=dict(n_frames=3, max_dist=30), note='cap at most 2048'),
    H=I(1, note='H, W >= 1 (not read with d_ctab)'), W=I(1),
    max_dist=I(1, None, note='1 <= max_dist <= 32767 and within the LDS (a relation: see the rules)'),
    conn8=FLAG,
    max_gap=I(1, 2, at_lo=dict(dmax=[9]), note='max_gap is 1 or 2'),
    thr_units=I(0, 1 << 46, note='0 <= thr_units <= 2^46'),
    t_begin=I(0, note='0 <= t_begin <= t_end <= n_frames'), t_end=I(None, None, note='t_begin <= t_end <= n_frames (a relation)')), [
    hw_rule(),
    Rule('t_begin <= t_end', refuse=dict(t_begin=3, t_end=2), limit=dict(t_begin=2, t_end=2)),
    Rule('t_end <= n_frames', refuse=dict(n_frames=4, t_end=5), limit=dict(n_frames=4, t_end=4)),
    Rule('n_frames * cap <= 2^30 - 1', refuse=dict(n_frames=1 << 20, cap=1 << 10, t_end=1), limit=dict(n_frames=1 << 10, cap=8, t_end=1 << 10),
         gap='2^30 - 1 slots need 16 GiB of d_pred and d_work: run at 2^10 frames x 8'),
    Rule('66 cap + 48 cap (cap <= 576) + 8 max_dist + 32 <= 163840 bytes of LDS', refuse=dict(cap=8, max_dist=HUNG_MAX_DIST_CAP8 + 1),
         limit=dict(cap=8, max_dist=HUNG_MAX_DIST_CAP8, dmax=[9, 5])),
    Rule('max_dist <= 32767', refuse=dict(cap=8, max_dist=40000)),
    Rule('0 <= h_dmax[g] <= 32767: below', refuse=dict(dmax=[9, -1])),
    Rule('0 <= h_dmax[g] <= 32767: above', refuse=dict(dmax=[32768, 5])),
    Rule('h_dmax[g] > max_dist stays accepted on the closed form (grid = NULL)', refuse=None, limit=dict(max_dist=30, dmax=[40, 35]))])
def _hungarian_pairs(n_frames=4, cap=8, H=64, W=64, max_dist=30, conn8=0, max_gap=2, dmax=None, thr_units=700000, t_begin=0, t_end=None):
    t_end = n_frames if t_end is None else t_end
    dmax = np.array([9, 5][:max(max_gap, 1)] if dmax is None else dmax, i32)
    F_, g_ = max(n_frames, 1), max(max_gap, 1)
    count, x, y = _dets(F_, cap, H, W, 22)
    slots = F_ * max(cap, 1)
    return [('d_x', x), ('d_y', y), ('d_count', count),
            ('n_frames', n_frames), ('cap', cap), ('grid', None), ('H', H), ('W', W), ('max_dist', max_dist), ('conn8', conn8),
            ('max_gap', max_gap), ('h_dmax', Host(dmax)),
            ('d_cost_units', Dev(data=_units(g_, max_dist)) if not _lazy((g_, max_dist)) else Dev((g_, max_dist + 1), i64)),
            ('thr_units', thr_units), ('t_begin', t_begin), ('t_end', t_end), ('d_pred', Dev((2, slots), i32, out=True)),
            ('d_work', Dev((2 * slots + F_ + 1,), i32, out=True)), ('stream', None), ('d_ctab', None)]


@register('axt_chain_tracks', dict(n_frames=I(1, note='n_frames >= 1'), cap=I(1, note='cap >= 1')), [
    Rule('n_frames * cap <= 2^30 - 1', refuse=dict(n_frames=1 << 20, cap=1 << 10), limit=dict(n_frames=1 << 12, cap=8),
         gap='2^30 - 1 slots need 20 GiB: run at 2^12 frames x 8')])
def _chain_tracks(n_frames=3, cap=4):
    F_ = max(n_frames, 1)
    count, _, _ = _dets(F_, cap, 9, 9, 1, per_frame=2)
    slots = F_ * max(cap, 1)
    return [('d_count', count), ('n_frames', n_frames), ('cap', cap), ('d_pred', Dev((2, slots), i32, fill=-1)),
            ('d_work', Dev((2 * slots,), i32, out=True)), ('d_track', Dev((slots,), i32, out=True)), ('d_n_tracks', Dev((1,), i32, out=True)),
            ('stream', None)]


@register('axt_ided_table', dict(
    n_frames=I(1, note='n_frames >= 1'), cap=I(1, note='cap >= 1'), n_ids=I(0, at_lo=dict(n_rows=0), note='n_ids >= 0'),
    n_rows=I(0, at_lo=dict(n_ids=0), note='n_rows >= 0, and n_rows == n_ids without d_id_row'),
    label_quirk=FLAG), [
    Rule('n_rows == n_ids without d_id_row', refuse=dict(n_ids=3, n_rows=2)),
    Rule('n_frames * cap <= 2^31 - 1', refuse=dict(n_frames=1 << 16, cap=1 << 15), limit=dict(n_frames=1 << 10, cap=1 << 10),
         gap='2^31 - 1 slots need 32 GiB of detections: run at 2^10 x 2^10'),
    Rule('n_rows * n_frames <= 2^31 - 1', refuse=dict(n_frames=1 << 16, cap=1, n_ids=1 << 15, n_rows=1 << 15),
         limit=dict(n_frames=1 << 10, cap=1, n_ids=1 << 10, n_rows=1 << 10), gap='2^31 - 1 rows x frames are 48 GiB of table: run at 2^10 x 2^10')])
def _ided_table(n_frames=3, cap=4, n_ids=2, n_rows=2, label_quirk=0):
    F_ = max(n_frames, 1)
    count, x, y = _dets(F_, cap, 9, 9, 1, per_frame=2)
    track = lambda: np.tile(np.arange(max(cap, 1), dtype=i32) % max(n_ids, 1), (F_, 1)) if n_ids > 0 else np.full((F_, cap), -1, i32)
    return [('d_track', _in((F_, cap), i32, track)), ('d_conf', Dev((F_, cap), f32, fill=0.75)), ('d_x', x),
            ('d_y', y), ('d_count', count), ('n_frames', n_frames), ('cap', cap), ('n_ids', n_ids),
            ('d_id_row', None), ('n_rows', n_rows), ('label_quirk', label_quirk), ('d_work', Dev((F_,), i32, out=True)),
            ('d_table', Dev((max(n_rows, 1), 3 * F_), f64, out=True)), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- reconstructions
@register('axt_track_links', dict(
    n_frames=I(0, note='n_frames == 0: AXT_OK and *n_links = 0'), cap=I(1, note='cap >= 1'),
    max_gap=I(1, 255, at_hi=dict(cap=8), note='1 <= max_gap <= 255')), [
    Rule('n_frames * cap <= 2^30 - 1', refuse=dict(n_frames=1 << 20, cap=1 << 10), limit=dict(n_frames=1 << 12, cap=8),
         gap='2^30 - 1 slots need 24 GiB: run at 2^12 frames x 8')])
def _track_links(n_frames=5, cap=4, max_gap=2):
    F_ = max(n_frames, 0)
    count, _, _ = _dets(F_, cap, 9, 9, 1, per_frame=3)
    track = lambda: (np.arange(max(cap, 1), dtype=i32)[None] + (np.arange(F_, dtype=i32)[:, None] % 3 == 1) * 100)      # every third frame misses
    slots = F_ * max(cap, 1)
    return [('d_track', _in((F_, cap), i32, track)), ('d_count', count), ('n_frames', n_frames), ('cap', cap), ('max_gap', max_gap),
            ('d_links', Dev((max(slots, 1), 3), i32, out=True)), ('d_work', Dev((2 * slots + 2 * F_ + 1,), i32, out=True)),
            ('n_links', Host(np.array([-77], i64), out=True)), ('stream', None)]


@register('axt_link_paths', dict(
    cap=I(1, note='cap >= 1'), n_links=I(0, note='n_links >= 0'),
    group=GROUP,
    H=I(1), W=I(1), max_dist=I(2, 32767, at_hi=dict(n_links=2), note='2 <= max_dist <= 32767'), conn8=FLAG),
    [hw_rule()])
def _link_paths(cap=4, n_links=3, group=0, H=40, W=50, max_dist=30, conn8=0):
    count, x, y = _dets(3, cap, H, W, 6, per_frame=4)
    n = max(n_links, 0)
    links = lambda: np.stack([np.arange(n) % max(cap, 1), max(cap, 1) + np.arange(n) % max(cap, 1), np.ones(n)], 1)
    return [('grid', None), ('d_x', x), ('d_y', y), ('cap', cap),
            ('d_links', _in((n, 3), i32, links)), ('n_links', n_links), ('d_head_group', None), ('group', group), ('H', H), ('W', W),
            ('max_dist', max_dist), ('conn8', conn8), ('d_len', Dev((max(n, 1),), i32, out=True)), ('d_stage', Dev((max(n, 1), max_dist), i32, out=True)),
            ('stream', None)]


@register('axt_link_cells', dict(
    n_links=I(0, note='n_links >= 0'), max_dist=I(2, 32767, note='2 <= max_dist <= 32767'),
    max_gap=I(1, 255, note='1 <= max_gap <= 255')))
def _link_cells(n_links=3, max_dist=30, max_gap=2):
    n = max(n_links, 0)
    lens = lambda: np.where(np.arange(max(n, 1)) % 3 == 2, max_dist, np.arange(max(n, 1)) % min(max_dist, 7))       # every third: no path
    return [('d_links', Dev((max(n, 1), 3), i32, fill=1)), ('n_links', n_links), ('d_len', _in((max(n, 1),), i32, lens)),
            ('d_stage', Dev((max(n, 1), max(max_dist, 1)), i32)), ('max_dist', max_dist), ('max_gap', max_gap),
            ('d_cell_ptr', Dev((n + 1,), i64, out=True)), ('d_cells', None), ('d_interp', None), ('n_cells', Host(np.array([-77], i64), out=True)),
            ('stream', None)]


# ----------------------------------------------------------------------------------------------------- target screens
@register('axt_target_field', dict(H=I(1), W=I(1), conn8=FLAG, n_targets=I(1, note='n_targets >= 1')), [hw_rule()])
def _target_field(H=20, W=30, conn8=0, n_targets=2):
    n = max(n_targets, 1)
    return [('grid', None), ('H', H), ('W', W), ('conn8', conn8), ('d_target_cells', _in((n,), i32, lambda: np.arange(n) * 7 % max(H * W, 1))),
            ('n_targets', n_targets), ('d_off', Dev((H, W), i32, out=True)), ('d_moves', Dev((H, W), i32, out=True)),
            ('n_rounds', Host(np.array([-9], i32), out=True)), ('stream', None)]


@register('axt_target_sample', dict(
    n_fields=I(1, at_lo={}, note='n_fields >= 1'), H=I(1), W=I(1), n_frames=I(0, note='n_frames == 0: AXT_OK, nothing is touched'),
    cap=I(1, note='cap >= 1')), [
    hw_rule(),
    Rule('n_frames * cap <= 2^31 - 1', refuse=dict(n_frames=1 << 16, cap=1 << 15), limit=dict(n_frames=1 << 10, cap=1 << 10),
         gap='2^31 - 1 slots need 32 GiB: run at 2^10 x 2^10')])
def _target_sample(n_fields=1, H=20, W=30, n_frames=2, cap=4):
    F_ = max(n_frames, 0)
    count, x, y = _dets(F_, cap, H, W, 8, per_frame=3)
    nf = max(n_fields, 1)
    field = lambda k: _in((nf, H, W), i32, lambda: (np.arange(nf * H * W).reshape(nf, H, W) * k) % 1009)
    return [('d_off', field(3)), ('d_moves', field(7)), ('n_fields', n_fields),
            ('d_field_index', Dev((max(F_, 1),), i32) if n_fields != 1 else None), ('H', H), ('W', W), ('d_x', x),
            ('d_y', y), ('d_count', count), ('n_frames', n_frames), ('cap', cap),
            ('d_det_off', Dev((F_, cap), i32, out=True)), ('d_det_moves', Dev((F_, cap), i32, out=True)), ('stream', None)]


@register('axt_target_paths', dict(
    H=I(1), W=I(1), conn8=FLAG, n_frames=I(0, note='n_frames >= 0'), cap=I(1, note='cap >= 1'),
    group=GROUP), [
    hw_rule(),
    Rule('n_frames * cap <= 2^31 - 1', refuse=dict(n_frames=1 << 16, cap=1 << 15), limit=dict(n_frames=1 << 10, cap=1 << 10),
         gap='2^31 - 1 slots need 24 GiB: run at 2^10 x 2^10')])
def _target_paths(H=20, W=30, conn8=0, n_frames=2, cap=4, group=0):
    F_ = max(n_frames, 0)
    count, x, y = _dets(F_, cap, H, W, 8, per_frame=3)
    slots = F_ * max(cap, 1)
    return [('grid', None), ('d_off', Dev((H, W), i32)), ('d_moves', Dev((H, W), i32)), ('H', H), ('W', W), ('conn8', conn8),
            ('d_x', x), ('d_y', y), ('n_frames', n_frames), ('cap', cap),
            ('d_det_moves', _in((max(slots, 1),), i32, lambda: np.arange(max(slots, 1)) % 5 - 1)), ('d_field_index', None), ('group', group),
            ('d_cell_ptr', Dev((slots + 1,), i64, out=True)), ('d_cells', None), ('n_cells', Host(np.array([-77], i64), out=True)), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- mask preparation
@register('axt_segment_edges', dict(
    H=I(None, None, note='min(H, W) >= 2 radius + 2 (a relation)'), W=I(None, None),
    sigma=F(lo=float(np.nextafter(0.0, 1.0)), hi=4.124, below=0.0, above=4.13, at_lo={}, at_hi=dict(H=40, W=40),
            note='sigma > 0 and radius = int(4 sigma + 0.5) <= 16')), [
    hw_rule(sigma=0.5),
    Rule('min(H, W) >= 2 radius + 2', refuse=dict(H=5, W=40, sigma=0.5), limit=dict(H=6, W=6, sigma=0.5))])
def _segment_edges(H=12, W=14, sigma=0.5):
    img = lambda: np.random.default_rng(1).integers(0, 65535, (H, W))
    return [('d_img', _in((H, W), u16, img)), ('H', H), ('W', W), ('sigma', sigma), ('d_P', Dev((H, W), f32, out=True)),
            ('d_G', Dev((H, W), f32, out=True)), ('d_minmax', Dev((2,), f32, out=True)), ('stream', None)]


@register('axt_segment_histogram', dict(
    n=I(1, INT_MAX, run_hi=1 << 22, gap='n = 2^31 - 1 needs 8 GiB: run at 2^22', note='1 <= n <= 2^31 - 1'),
    mn=F(lo=-3.5e38, below=-1e39, note='mn <= mx finite'), mx=F(hi=3.5e38, above=1e39, at_hi=dict(mn=0.0))), [
    Rule('mn <= mx', refuse=dict(mn=2.0, mx=1.0), limit=dict(mn=1.0, mx=1.0))])
def _segment_histogram(n=64, mn=0.0, mx=1.0):
    return [('d_G', _in((max(n, 1),), f32, lambda: np.linspace(0, 1, max(n, 1)))), ('n', n), ('mn', mn), ('mx', mx),
            ('d_hist', Dev((256,), i64, out=True)), ('stream', None)]


@register('axt_segment_close', dict(
    H=I(1), W=I(1), thr=F(inf_ok=True, note='thr a number'), k=I(2, 32, note='2 <= k <= 32')), [hw_rule()])
def _segment_close(H=12, W=14, thr=0.5, k=3):
    return [('d_P', _in((H, W), f32, lambda: np.random.default_rng(2).uniform(0, 1, (H, W)))), ('H', H), ('W', W), ('thr', thr), ('k', k),
            ('d_out', Dev((H, W), u8, out=True)), ('stream', None)]


@register('axt_segment_flood', dict(
    H=I(1, at_lo=dict(seed_y=0)), W=I(1, at_lo=dict(seed_x=0)), seed_y=I(0, None, note='0 <= seed_y < H'), seed_x=I(0, None, note='0 <= seed_x < W'),
    conn8=FLAG), [
    hw_rule(),
    Rule('seed_y < H', refuse=dict(H=12, seed_y=12), limit=dict(H=12, seed_y=11)),
    Rule('seed_x < W', refuse=dict(W=14, seed_x=14), limit=dict(W=14, seed_x=13))])
def _segment_flood(H=12, W=14, seed_y=3, seed_x=4, conn8=0):
    return [('d_img', _in((H, W), u8, lambda: np.random.default_rng(3).integers(0, 2, (H, W)))), ('H', H), ('W', W), ('seed_y', seed_y),
            ('seed_x', seed_x), ('conn8', conn8), ('d_out', Dev((H, W), u8, out=True)), ('rounds_out', Host(np.array([-9], i32), out=True)),
            ('stream', None)]


# ----------------------------------------------------------------------------------------------------- metrics, scores
@register('axt_detection_confusion', dict(
    n_frames=I(1, note='n_frames >= 1'), cap=I(1, 2048, at_hi=dict(n_frames=1), note='1 <= cap <= 2048'),
    gcap=I(1, note='gcap >= 1'), n_thr=I(1, 65535, at_hi=dict(n_frames=1, cap=2, gcap=2), note='1 <= n_thr <= 65535'),
    min_dist=I(0, 1024, note='0 <= min_dist <= 1024'),
    k_mask=I(None, None, note='any k_mask < 0 means no masks; k_mask < n_thr (a relation)')), [
    Rule('k_mask < n_thr', refuse=dict(n_thr=3, k_mask=3), limit=dict(n_thr=3, k_mask=2))])
def _detection_confusion(n_frames=2, cap=4, gcap=3, n_thr=3, min_dist=23, k_mask=-1):
    F_ = max(n_frames, 1)
    count, x, y = _dets(F_, cap, 60, 60, 12, per_frame=3)
    gcount, gx, gy = _dets(F_, gcap, 60, 60, 13, per_frame=2)
    masks = k_mask >= 0
    return [('d_conf', _in((F_, cap), f32, lambda: np.random.default_rng(1).uniform(0.5, 1, (F_, cap)))), ('d_x', x),
            ('d_y', y), ('d_count', count), ('n_frames', n_frames), ('cap', cap),
            ('d_gx', gx), ('d_gy', gy), ('d_gcount', gcount), ('gcap', gcap),
            ('d_thrs', _in((max(n_thr, 1),), f64, lambda: np.linspace(0.5, 0.9, max(n_thr, 1)))), ('n_thr', n_thr), ('min_dist', min_dist),
            ('k_mask', k_mask), ('d_confusion', Dev((F_, 3, max(n_thr, 1)), i32, out=True)),
            ('d_fp_mask', Dev((F_, cap), u8, out=True) if masks else None), ('d_fn_mask', Dev((F_, gcap), u8, out=True) if masks else None),
            ('stream', None)]


def mot_scratch(no, nh, n_assoc):
    """mot.hip: the bytes of scratch axt_mot_scores asks for while the identity matching fits the LDS (small no, nh)."""
    r8 = lambda v: (v + 7) & ~7
    return (r8(no * nh * 4) + r8(no * 4) + r8(no)) * n_assoc


@register('axt_mot_scores', dict(
    n_assoc=I(1, 65535, at_hi=dict(n_frames=1, cap=1, gcap=1, no=1, nh=1), note='1 <= n_assoc <= 65535'),
    n_frames=I(1, note='n_frames >= 1'),
    cap=I(1, 1024, at_hi=dict(n_frames=1), note='cap, gcap <= 1024'), gcap=I(1, 1024, at_hi=dict(n_frames=1)),
    no=I(1, 1 << 24, run_hi=64, gap='no = 2^24 needs 64 MiB of tallies per association and a matching of that size: run the size query at the bound, the kernels at 64',
         note='no, nh <= 2^24'),
    nh=I(1, 1 << 24, run_hi=64, gap='as no'), max_dist=I(0, 255, note='max_dist <= 255')), [
    Rule('*scratch_bytes (in) >= the size the query answers', refuse=dict(scratch=8))])
def _mot_scores(n_assoc=1, n_frames=2, cap=3, gcap=3, no=2, nh=2, max_dist=10, scratch=None):
    F_ = max(n_frames, 1)
    count, x, y = _dets(F_, cap, 50, 50, 14, per_frame=2)
    gcount, gx, gy = _dets(F_, gcap, 50, 50, 14, per_frame=2)
    A = max(n_assoc, 1)
    ids = lambda n, lim: np.tile(np.where(np.arange(max(n, 1)) < lim, np.arange(max(n, 1)), -1).astype(i32), (F_, 1))      # unique in a frame
    need = mot_scratch(max(no, 1), max(nh, 1), A)
    return [('d_track', _in((A, F_, cap), i32, lambda: np.tile(ids(cap, nh), (A, 1, 1)))), ('n_assoc', n_assoc), ('d_x', x),
            ('d_y', y), ('d_count', count), ('n_frames', n_frames), ('cap', cap),
            ('d_gid', _in((F_, gcap), i32, lambda: ids(gcap, no))), ('d_gx', gx), ('d_gy', gy),
            ('d_gcount', gcount), ('gcap', gcap), ('no', no), ('nh', nh), ('max_dist', max_dist),
            ('d_counts', Dev((A, 10), i64, out=True)), ('d_tallies', Dev((A, max(no, 1), 2), i32, out=True)), ('d_ev_kind', None),
            ('d_ev_partner', None), ('d_ev_fp', None), ('d_scratch', Dev((max(need, 8),), u8, out=True)),
            ('scratch_bytes', Host(np.array([need if scratch is None else scratch], np.uintp), out=True, written_on_refusal=scratch is not None)),
            ('stream', None)]


# ----------------------------------------------------------------------------------------------------- rendering
RT = 64


@register('axt_render_frames', dict(
    mask_stride=I(0, note='mask_stride >= 0'), n_out=I(0, note='n_out == 0: AXT_OK, nothing is touched; negative: AXT_EINVAL'),
    H=I(1, at_lo=dict(Ho=1)), W=I(1, at_lo=dict(Wo=1)), ymin=I(0, note='ymin, xmin >= 0'), xmin=I(0), Ho=I(1, note='Ho, Wo >= 1'), Wo=I(1),
    grid=I(0, note='grid >= 0'),
    bg=FLAG), [
    hw_rule(),
    Rule('ymin + Ho <= H', refuse=dict(H=64, ymin=1, Ho=64), limit=dict(H=65, ymin=1, Ho=64)),
    Rule('xmin + Wo <= W', refuse=dict(W=64, xmin=1, Wo=64), limit=dict(W=65, xmin=1, Wo=64)),
    Rule('ymin + Ho computed without overflow', refuse=dict(H=64, ymin=INT_MAX, Ho=64)),
    Rule('n_out * tiles < 2^31 - 1', refuse=dict(n_out=1 << 20, H=4096, W=4096, Ho=4096, Wo=4096), limit=dict(n_out=64, H=128, W=128, Ho=128, Wo=128),
         gap='2^31 - 2 (frame, tile) items need 24 TiB of output: run at 64 frames x 4 tiles')])
def _render_frames(mask_stride=0, n_out=2, H=64, W=64, ymin=0, xmin=0, Ho=64, Wo=64, grid=0, bg=0):
    n = max(n_out, 0)
    nt = cdiv(max(Wo, 1), RT) * cdiv(max(Ho, 1), RT)
    return [('d_frames', _in((max(n, 1), H, W), f32, lambda: np.random.default_rng(1).uniform(0, 1, (max(n, 1), H, W)))), ('d_mask', None),
            ('mask_stride', mask_stride), ('d_ts', _in((max(n, 1),), i32, lambda: np.arange(max(n, 1)))), ('n_out', n_out), ('H', H), ('W', W),
            ('ymin', ymin), ('xmin', xmin), ('Ho', Ho), ('Wo', Wo), ('grid', grid), ('bg', bg), ('d_trail_ptr', Dev((nt + 1,), i32)),
            ('d_trail', Dev((1, 4), i32)), ('d_trail_col', Dev((4,), u8)), ('d_prim_ptr', Dev((n * nt + 1,), i32)), ('d_prims', Dev((1, 8), i32)),
            ('d_tables', Dev((60 + 95 * 7,), u8, fill=0x15)), ('d_out', Dev((n, Ho, Wo, 3), u8, out=True)), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- training helpers
@register('axt_yolo_targets', dict(
    F=I(0, note='F >= 0 (F == 0 writes nothing)'), cap=I(1, note='cap >= 1'),
    n_tiles=I(1, 256, note='1 <= n_tiles <= 256')), [
    Rule('tile indices 0 .. 32766: below', refuse=dict(tiles=[(0, -1)], n_tiles=1)),
    Rule('tile indices 0 .. 32766: above', refuse=dict(tiles=[(32767, 0)], n_tiles=1), limit=dict(tiles=[(32766, 32766)], n_tiles=1)),
    Rule('F * n_tiles * 144 < 2^39', refuse=dict(F=INT_MAX, n_tiles=256), limit=dict(F=64, n_tiles=256),
         gap='2^39 cells are 8 TiB of targets: run at 64 frames x 256 tiles')])
def _yolo_targets(F=2, cap=4, n_tiles=2, tiles=None):
    F_ = max(F, 0)
    t = _tiles(n_tiles) if tiles is None else np.array(tiles, i32)
    count, x, y = _dets(F_, cap, 600, 600, 15, per_frame=3)
    return [('d_lx', x), ('d_ly', y), ('d_lcount', count), ('F', F), ('cap', cap),
            ('h_tile_yx', Host(t)), ('n_tiles', n_tiles), ('d_target', Dev((F_, n_tiles, 12, 12, 4), f32, out=True)), ('stream', None)]


_POOL_ROWS = dict(
    n_maps=I(0, note='n_maps = 0 does nothing'), H=I(2, 32768, at_hi=dict(n_maps=1, W=2), note='2 <= H, W <= 32768'),
    W=I(2, 32768, at_hi=dict(n_maps=1, H=2)))
_POOL_RULES = [Rule('n_maps * H * W <= 2^38', refuse=dict(n_maps=(1 << 28) + 1, H=32, W=32), limit=dict(n_maps=1 << 12, H=32, W=32),
                    gap='2^38 elements are 1 TiB: run at 2^12 maps of 32 x 32')]


@register('axt_maxpool2_forward', _POOL_ROWS, _POOL_RULES)
def _maxpool2_forward(n_maps=3, H=6, W=5):
    n = max(n_maps, 0)
    return [('d_in', _in((n, H, W), f32, lambda: np.random.default_rng(1).normal(size=(n, H, W)))), ('n_maps', n_maps), ('H', H), ('W', W),
            ('d_out', Dev((n, max(H, 0) // 2, max(W, 0) // 2), f32, out=True)), ('stream', None)]


@register('axt_maxpool2_backward', _POOL_ROWS, _POOL_RULES)
def _maxpool2_backward(n_maps=3, H=6, W=5):
    n = max(n_maps, 0)
    return [('d_in', _in((n, H, W), f32, lambda: np.random.default_rng(1).normal(size=(n, H, W)))),
            ('d_dout', Dev((n, max(H, 0) // 2, max(W, 0) // 2), f32, fill=1.0)), ('n_maps', n_maps), ('H', H), ('W', W),
            ('d_din', Dev((n, H, W), f32, out=True)), ('stream', None)]


@register('axt_tile_stacks', dict(
    T_all=I(None, None, note='t0 + n_frames + 4 <= T_all (a relation)'), H=I(1, 32768, at_hi=dict(W=4), note='1 <= H, W <= 32768'),
    W=I(1, 32768, at_hi=dict(H=4)), t0=I(0, note='t0 >= 0'),
    n_frames=I(1, 1 << 22, at_hi=lambda v: dict(T_all=v + 4, t0=0, H=1, W=1), note='1 <= n_frames <= 2^22'),
    n_tiles=I(1, 256, at_hi=lambda v: dict(tiles=[(0, 0)] * v), note='1 <= n_tiles <= 256'),
    B=I(1, 1024, run_hi=64, gap='B = 1024 writes 5 GiB of stacks: run at 64', note='1 <= B <= 1024')), [
    Rule('t0 + n_frames + 4 <= T_all', refuse=dict(T_all=6, t0=1, n_frames=2), limit=dict(T_all=7, t0=1, n_frames=2)),
    Rule('tile origins inside the frame: negative', refuse=dict(tiles=[(-1, 0)], n_tiles=1)),
    Rule('tile origins inside the frame: beyond', refuse=dict(tiles=[(0, 1)], n_tiles=1, W=512), limit=dict(tiles=[(0, 1)], n_tiles=1, W=513)),
    Rule('tile origins inside the frame: an index whose product with 512 wraps', refuse=dict(tiles=[(4194304, 0)], n_tiles=1))])
def _tile_stacks(T_all=7, H=20, W=24, t0=1, n_frames=2, n_tiles=1, B=2, tiles=None):
    t = _tiles(n_tiles) if tiles is None else np.array(tiles, i32)
    return [('d_frames', _in((T_all, H, W), f32, lambda: np.random.default_rng(1).uniform(0, 1, (T_all, H, W)))), ('T_all', T_all), ('H', H),
            ('W', W), ('t0', t0), ('n_frames', n_frames), ('h_tile_yx', Host(t)), ('n_tiles', n_tiles),
            ('d_index', _in((max(B, 1),), i32, lambda: np.arange(max(B, 1)) % max(n_frames * n_tiles, 1))), ('B', B),
            ('d_out', Dev((max(B, 0), 5, 512, 512), f32, out=True)), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- TIFF, JPEG
@register('axt_tiff_decode_u16', dict(
    src_len=I(0, note='a negative size'), n_segs=I(0, note='n_segs == 0 launches nothing'), W=I(0, note='a negative size'),
    compression=I(None, None, note='compression 1, 5 or 32773 (a set)'), predictor=I(1, 2, note='predictor 1 or 2'),
    big_endian=FLAG, out_len=I(0, note='a negative size')), [
    Rule('compression is one of 1, 5, 32773: 0', refuse=dict(compression=0), limit=dict(compression=1)),
    Rule('compression is one of 1, 5, 32773: 6', refuse=dict(compression=6), limit=dict(compression=5)),
    Rule('compression is one of 1, 5, 32773: 32774', refuse=dict(compression=32774), limit=dict(compression=32773))])
def _tiff_decode_u16(src_len=16, n_segs=1, W=4, compression=1, predictor=1, big_endian=0, out_len=8):
    seg = np.zeros(max(n_segs, 1) * 4, i64)                  # src_offset, src_bytes, dst_offset, rows | reserved
    seg[0:3] = (0, 16, 0)
    seg[3] = 2                                               # rows = 2 in the low half, reserved = 0
    return [('d_src', Dev((max(src_len, 1),), u8, fill=1)), ('src_len', src_len), ('d_segs', Dev(data=seg)), ('n_segs', n_segs), ('W', W),
            ('compression', compression), ('predictor', predictor), ('big_endian', big_endian), ('d_out', Dev((max(out_len, 1),), u16, out=True)),
            ('out_len', out_len), ('d_status', Dev((max(n_segs, 1),), i32, out=True, fill=-1)), ('stream', None)]


_JPEG_DIM = I(1, 65535, note='H or W outside 1..65535')
register('axt_jpeg_scan_bound', dict(H=_JPEG_DIM, W=_JPEG_DIM))(lambda H=16, W=16: [('H', H), ('W', W)])
register('axt_jpeg_scratch_bytes', dict(n_frames=I(0, note='a negative size'), H=_JPEG_DIM, W=_JPEG_DIM))(
    lambda n_frames=1, H=16, W=16: [('n_frames', n_frames), ('H', H), ('W', W)])


LIB = None          # the loaded library, set by whoever runs the calls: the JPEG builder asks it for the scratch size


def jpeg_scratch(n_frames, H, W):
    n = int(LIB.axt_jpeg_scratch_bytes(n_frames, H, W)) if LIB is not None else -1
    return n if n > 0 else 1 << 16


@register('axt_jpeg_encode_rgb8', dict(
    n_frames=I(0, note='n_frames == 0 launches nothing'), H=I(1, 65535, at_hi=dict(W=8, n_frames=1), note='H or W outside 1..65535'),
    W=I(1, 65535, at_hi=dict(H=8, n_frames=1)), frame_stride=I(None, None, note='frame_stride >= 3 * H * W (a relation)'),
    quality=I(1, 100, note='a quality outside 1..100'), scan_capacity=I(0, note='a negative size'),
    scratch_bytes=I(None, None, note='scratch that is smaller than the query (a relation)')), [
    Rule('frame_stride >= 3 * H * W', refuse=dict(H=16, W=16, frame_stride=767), limit=dict(H=16, W=16, frame_stride=768)),
    Rule('scratch_bytes >= axt_jpeg_scratch_bytes(n_frames, H, W)', refuse=dict(scratch_bytes=16)),
    Rule('n_frames * ceil(H / 8) * ceil(W / 8) < 2^31', refuse=dict(n_frames=1 << 10, H=16384, W=16384, frame_stride=3 << 28,
                                                                    scratch_bytes=1 << 50))])
def _jpeg_encode_rgb8(n_frames=1, H=16, W=16, frame_stride=None, quality=90, scan_capacity=1 << 16, scratch_bytes=None):
    stride = 3 * H * W if frame_stride is None else frame_stride
    n = max(n_frames, 1)
    need = jpeg_scratch(n_frames, H, W)
    scratch = need if scratch_bytes is None else scratch_bytes
    return [('d_rgb', _in((n, H, W, 3), u8, lambda: np.random.default_rng(1).integers(0, 255, (n, H, W, 3)))), ('n_frames', n_frames), ('H', H),
            ('W', W), ('frame_stride', stride), ('quality', quality), ('d_scan', Dev((n, max(scan_capacity, 1)), u8, out=True)),
            ('scan_capacity', scan_capacity), ('d_scan_bytes', Dev((n,), i64, out=True)), ('d_status', Dev((n,), i32, out=True)),
            ('d_scratch', Dev((need,), u8, out=True)), ('scratch_bytes', scratch), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- augmentation
_ANY_SHIFT = 'dy, dx (any sign and size)'
_MATRIX = F(at_lo=dict(rotate=1), note='m00 .. m11 finite when rotate != 0 (not read otherwise)')


@register('axt_augment_frames', dict(
    T=I(1, 65535 * 6, at_hi=dict(H=1, W=1), note='1 <= T <= 393210'),
    H=I(1, 65535 * 4, at_hi=dict(W=1, T=1), note='1 <= H <= 262140'), W=I(1), dy=free(_ANY_SHIFT), dx=free(_ANY_SHIFT),
    flip_y=FLAG, flip_x=FLAG, rotate=FLAG,
    m00=_MATRIX, m01=_MATRIX, m10=_MATRIX, m11=_MATRIX), [hw_rule()])
def _augment_frames(T=2, H=6, W=8, dy=1, dx=-1, flip_y=0, flip_x=1, rotate=0, m00=1.0, m01=0.0, m10=0.0, m11=1.0):
    return [('d_in', _in((T, H, W), f32, lambda: np.random.default_rng(1).uniform(0, 1, (T, H, W)))), ('T', T), ('H', H), ('W', W), ('dy', dy),
            ('dx', dx), ('flip_y', flip_y), ('flip_x', flip_x), ('rotate', rotate), ('m00', m00), ('m01', m01), ('m10', m10), ('m11', m11),
            ('d_out', Dev((T, H, W), f32, out=True)), ('d_occ', None), ('stream', None)]


# ----------------------------------------------------------------------------------------------------- handle-taking entry points
_FRAMES_ROWS = dict(
    T_all=I(None, None, note='t0 + n_frames + 4 <= T_all (a relation)'), H=I(1), W=I(1), t0=I(0), n_frames=I(0),
    n_tiles=I(1, 256, note='1 <= n_tiles <= 256'))
register('axt_detector_create', dict(n_tensors=I(54, 54, note='h_tensors[54]'), max_batch=I(1, 65535, note='1 <= max_batch <= 65535')), handle='detector')
for _n in ('axt_detector_destroy', 'axt_detector_device_bytes', 'axt_grid_destroy', 'axt_head_trainer_destroy', 'axt_head_trainer_device_bytes',
           'axt_head_trainer_read_weights', 'axt_conv_trainer_destroy', 'axt_conv_trainer_device_bytes', 'axt_conv_trainer_read_weights',
           'axt_conv_trainer_read_stats', 'axt_head_trainer_export'):
    register(_n, {}, handle=_n.split('_')[1] if 'trainer' not in _n else 'trainer')
register('axt_detector_set_arith', dict(mode=I(0, 2, note='mode 0, 1 or 2')), handle='detector')
register('axt_detector_set_fused_front', dict(fused=I(0, 1, note='fused 0 or 1')), handle='detector')
register('axt_cnn_forward', dict(B=I(0, None, note='0 <= B <= max_batch')), handle='detector')
register('axt_cnn_forward_frames', _FRAMES_ROWS, handle='detector')
register('axt_cnn_features_frames', _FRAMES_ROWS, handle='detector')
register('axt_cnn_block_features_frames', dict(_FRAMES_ROWS, block=I(2, 7, note='block 2, 4, 6 or 7; any other block: AXT_EINVAL')), handle='detector')
register('axt_cnn_front_frames', dict(_FRAMES_ROWS, item0=I(0, None, note='item0 + items <= max_batch')), handle='detector')
register('axt_cnn_back', dict(n_items=I(0, None, note='0 <= n_items <= max_batch')), handle='detector')
register('axt_detector_set_profiling', dict(on=free('on is not range-checked')), handle='detector')
register('axt_detector_read_profile', dict(n=I(14, None, note='n >= AXT_N_CNN_KERNELS')), handle='detector')
register('axt_grid_create', dict(H=I(1), W=I(1), conn8=FLAG), handle='grid (made by this call, which uploads it)')
register('axt_head_trainer_create', dict(K0=I(1), H1=I(1), H2=I(1), NOUT=I(432, 432, note='NOUT = 432'), max_batch=I(1, 64, note='max_batch <= 64')),
         handle='trainer')
register('axt_head_trainer_read_moments', dict(layer=I(0, 2, note='layer 0..2')), handle='trainer')
_B = I(1, 64, note='1 <= B <= max_batch')
_ADAM = dict(lr=free('lr and the three lambdas are taken as they are'), beta1=F(lo=0.0, hi=float(np.nextafter(1.0, 0.0)), below=-0.1, above=1.0),
             beta2=F(lo=0.0, hi=float(np.nextafter(1.0, 0.0)), below=-0.1, above=1.0), eps=F(lo=0.0, below=-1e-9), weight_decay=F(lo=0.0, below=-1e-9))
_LAMBDA = free('lr and the three lambdas are taken as they are')
register('axt_head_trainer_forward', dict(B=_B), handle='trainer')
register('axt_head_trainer_loss', dict(B=_B, lambda_obj=_LAMBDA, lambda_noobj=_LAMBDA, lambda_coord=_LAMBDA), handle='trainer')
register('axt_head_trainer_step', dict(_ADAM, B=_B), handle='trainer')
register('axt_head_trainer_input_grad', dict(B=_B), handle='trainer')
_CONV_CREATE = dict(Ci=I(1, 512, note='1 <= Ci, Co <= 512'), Co=I(1, 512), max_batch=I(1, 64, note='1 <= max_batch <= 64'))
register('axt_conv_trainer_create', dict(_CONV_CREATE, H=I(1, 64, note='1 <= H, W <= 64'), W=I(1, 64)), handle='trainer')
register('axt_conv_trainer_create_strided', dict(_CONV_CREATE, Hin=I(1, 512, note='1 <= Hin, Win <= 512'), Win=I(1, 512),
                                                 stride=I(1, 2, note='stride 1 or 2')), handle='trainer')
register('axt_conv_trainer_read_moments', dict(tensor=I(0, 3, note='tensor 0..3')), handle='trainer')
register('axt_conv_trainer_forward', dict(B=_B), handle='trainer')
register('axt_conv_trainer_step', dict(_ADAM, B=_B), handle='trainer')
register('axt_conv_trainer_input_grad', dict(B=_B), handle='trainer')
register('axt_conv_trainer_set_batch_stats', dict(on=FLAG,
                                                  momentum=F(lo=float(np.nextafter(0.0, 1.0)), hi=1.0, below=0.0, above=1.5, note='momentum in (0, 1]')),
         handle='trainer')
register('axt_detector_load_conv_block', dict(li=I(0, 7, note='conv block li (0..7')), handle='detector')
register('axt_detector_load_linear', dict(layer=I(0, 2, note='linear layer 0..2')), handle='detector')
register('axt_conv_trainer_export', dict(li=I(0, 7)), handle='trainer and detector')


# ===================================================================================================== derivation
class Call:
    """One complete call: `name` says what it probes, args the ordered (parameter, value) pairs of the builder."""

    def __init__(self, function, name, over, probe, gap=None):
        self.function, self.name, self.over, self.probe, self.gap = function, name, over, probe, gap

    @property
    def args(self):
        return call_args(self)

    @property
    def id(self):
        return f'{self.function}[{self.name}]'

    def __repr__(self):
        return self.id


def _over(extra, value):
    return dict(extra(value) if callable(extra) else extra)


def _fmt(v):
    return repr(v) if not isinstance(v, float) else f'{v:g}'


def refusals():
    out = []
    for fn in BUILDERS:
        for p, row in ROWS[fn].items():
            if isinstance(row, free):
                continue
            if row.below is not None:
                out.append(Call(fn, f'{p}={_fmt(row.below)}', dict(_over(row.beyond_lo, row.below), **{p: row.below}), p))
            if row.above is not None:
                out.append(Call(fn, f'{p}={_fmt(row.above)}', dict(_over(row.beyond_hi, row.above), **{p: row.above}), p))
            if row.kind == 'float':
                out.append(Call(fn, f'{p}=nan', dict(_over(row.at_lo, NAN), **{p: NAN}), p))
                if not row.inf_ok:
                    out.append(Call(fn, f'{p}=inf', dict(_over(row.at_lo, math.inf), **{p: math.inf}), p))
        for k, rule in enumerate(RULES[fn]):
            if rule.refuse is not None:
                out.append(Call(fn, f'rule {k}: {rule.text}', dict(rule.mode, **rule.refuse), rule.text))
    return out + LEGACY_REFUSALS


def limits():
    out = []
    for fn in BUILDERS:
        for p, row in ROWS[fn].items():
            if isinstance(row, free):
                continue
            if row.lo is not None:
                out.append(Call(fn, f'{p}={_fmt(row.lo)} (smallest)', dict(_over(row.at_lo, row.lo), **{p: row.lo}), p))
            if row.hi is not None:
                v = row.hi if row.run_hi is None else row.run_hi
                out.append(Call(fn, f'{p}={_fmt(v)} (largest{"" if row.run_hi is None else " that runs"})', dict(_over(row.at_hi, v), **{p: v}), p,
                                row.gap if row.run_hi is not None else None))
        for k, rule in enumerate(RULES[fn]):
            if rule.limit is not None:
                out.append(Call(fn, f'at rule {k}: {rule.text}', dict(rule.mode, **rule.limit), rule.text, rule.gap))
    return out


# The calls tests/test_host_logic.py used to make itself (it still asserts their codes and messages, through this list):
# (call, the fragment axt_last_error() must hold or None). _ptr replaces pointer arguments of the builder's call: None = NULL,
# 'P' = any pointer (never read: the checks come first).
def _legacy(fn, name, **over):
    return Call(fn, 'legacy: ' + name, over, name)


LEGACY = [
    (_legacy('axt_build_arcs', 'd_x NULL', _ptr=dict(d_x=None), max_dist=500), b'null argument'),
    (_legacy('axt_build_arcs', 'max_gap 9', max_gap=9, dmax=[0] * 9, max_dist=500), None),
    (_legacy('axt_build_arcs', 'histograms without their sums', _ptr=dict(d_hist='P'), vis_weight=0.5, max_dist=500), None),
    (_legacy('axt_build_arcs', 'weight 0', _ptr=dict(d_hist='P', d_hist_sum='P'), vis_weight=0.0, max_dist=500), None),
    (_legacy('axt_build_arcs', 'weight 1.5', _ptr=dict(d_hist='P', d_hist_sum='P'), vis_weight=1.5, max_dist=500), b'1.5'),
    (_legacy('axt_build_arcs', 'phase 2: costs wanted, no units', _ptr=dict(d_col='P', d_len='P', d_gap='P', d_cost='P', d_cost_units=None),
             max_dist=500), b'go together'),
    (_legacy('axt_hungarian_pairs', 'cap 2049', cap=2049, max_dist=500), b'2049'),
    (_legacy('axt_hungarian_pairs', 'max_gap 3', max_gap=3, dmax=[0, 0, 0], max_dist=500), None),
    (_legacy('axt_hungarian_pairs', 'frame range [3, 2)', t_begin=3, t_end=2, max_dist=500), None),
    (_legacy('axt_hungarian_pairs', 'neither a cost table nor units', _ptr=dict(d_cost_units=None), max_dist=500), None),
]
LEGACY_REFUSALS = [c for c, _ in LEGACY]


def call_args(call):
    """The (parameter, value) pairs of a call, pointer replacements of hand-written refusals applied."""
    over = dict(call.over)
    ptr = over.pop('_ptr', {})
    args = BUILDERS[call.function](**over)
    return [(n, (ptr[n] if n in ptr else v)) for n, v in args]


SENTINEL, REGION = 0xA5, 1 << 16


def sentinel_buffer():
    """One sentinel-filled region per pointer argument (entry points may compare two of them)."""
    return np.full(32 * REGION, SENTINEL, np.uint8)


def run_refusal(lib, call, sentinel):
    """Makes `call` on `lib` (a ctypes library with argtypes set) the way a refusal is made: every device pointer is the address of
    a sentinel-filled HOST region (never read: the checks come first), every host array the table's own. Returns the return
    code, axt_last_error() and whether a byte of either changed (host arrays the header lets a refused call write excepted)."""
    host, cargs = [], []
    for k, (_, v) in enumerate(call_args(call)):
        if isinstance(v, Dev) or (isinstance(v, str) and v == 'P'):
            cargs.append(sentinel.ctypes.data + k * REGION)
        elif isinstance(v, Host):
            a = v.data.copy()
            if not v.written_on_refusal:
                host.append((a, a.copy()))
            cargs.append(a.ctypes.data)
        else:
            cargs.append(v)
    import ctypes
    fn = getattr(lib, call.function)
    cargs = [ctypes.cast(ctypes.c_void_p(v), t) if isinstance(t, type) and issubclass(t, ctypes._Pointer) and v is not None else v
             for v, t in zip(cargs, fn.argtypes)]                            # (a binding may spell a pointer POINTER(c_int64))
    rc = fn(*cargs)
    msg = lib.axt_last_error().decode(errors='replace')
    touched = bool((sentinel != SENTINEL).any()) or any(not np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in host)
    sentinel[:] = SENTINEL
    return int(rc), msg, touched


# ===================================================================================================== what the device test leaves uncompared
EXACT_F64 = 1 << 37          # hungarian_reference.EXACT_F64: the costs its SciPy solver sums exactly


def uncompared(function, s):
    """Why tests/test_contract_gpu.py runs a limit call of `function` with the scalar arguments `s` for AXT_OK only, without
    comparing its outputs with the family's reference; None where it compares. The refusals that need a handle are in UNRUN."""
    if function == 'axt_build_arcs' and s.get('vis'):
        return ('the appearance term: its reference (stagekernel_cases.vis_csr) holds for cases whose costs keep a margin from the '
                'admission threshold, which a limit call does not arrange')
    if function == 'axt_hungarian_pairs' and (s['t_begin'], s['t_end']) != (0, s['n_frames']):
        return 'a partial frame range: hungarian_reference.judge takes the trajectories of a whole association'
    if function == 'axt_hungarian_pairs' and (s['thr_units'] << 16) >= EXACT_F64:
        return 'thr_units << 16 lies beyond the costs that hungarian_reference sums exactly in f64'
    if function == 'axt_detection_confusion' and s['n_thr'] > 64:
        return '65535 thresholds are 65535 passes of the oracle per frame'
    if function == 'axt_target_field' and s['H'] * s['W'] > 1 << 16:
        return 'target_reference.field is a Dijkstra over every cell: minutes at 2048 x 2048'
    return None


# Refusals the table states but no test makes: they need a grid, a grid needs a device, and out-of-contract calls stay off it.
UNRUN = [
    ('axt_hungarian_pairs', 'h_dmax[g] > max_dist with a grid (the closed form accepts it: see its limit call)'),
    ('axt_build_arcs', 'h_dmax[g] > max_dist with a grid and d_cost_units, without d_len_table (the d_len_table variant is refusal rule 4)'),
    ('axt_path_cost, axt_link_paths, axt_build_arcs, axt_hungarian_pairs, axt_target_field, axt_target_paths', 'a grid whose size is not H x W'),
]
