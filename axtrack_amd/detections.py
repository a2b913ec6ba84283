"""AxonDetections: the reference's orchestration class (axtrack/AxonDetections.py) re-hosted on
the HIP hot path. Same public surface on the inference path -- detect_dataset(), assign_ids(),
get_frame_dets(), IDed_dets_all, _detections, dir, name, len() -- but a timelapse is processed as
whole-array GPU passes instead of a Python loop over frames and DataFrames:

    detect_dataset : CNN forward for all (frame, kept tile) -> decode+stitch+NMS
    assign_ids     : observation costs + admissible-arc list on the GPU -> min-cost-flow solve (or the
                     frame-to-frame Hungarian variant) -> trajectories -> IDed_dets_all (filled on the GPU)
    compute_TP_FP_FN / get_detection_metrics : the evaluation metrics of labelled data, one launch

pandas objects are only materialised at the API boundary (lazily for the per-frame tables).
"""
import os
import re
import pickle

import numpy as np
import pandas as pd
import torch

from . import hotpath as hp


def transition_cost_table(P, max_px=hp.MAX_PX_ASSOC_DIST, vis_sim=0.0):
    """transition_model (mincostflow_models.py:67-119) tabulated for every integer path length
    D = 0..max_px and gap = 1..MCF_MAX_NUM_MISSES+1, numpy f64 exactly as the reference computes
    it, for one value of the visual similarity. Returns (cost f64 [gaps, max_px+1], dmax i32 [gaps]) with
    dmax = largest D whose cost < MCF_EDGE_COST_THR. With MCF_VIS_SIM_WEIGHT = 0 the table IS the cost model; with
    a weight the costs are computed per pair on the GPU (axt_build_arcs with d_hist) and the table for vis_sim = 1 only
    bounds the candidate pairs."""
    w = P['MCF_VIS_SIM_WEIGHT']
    gaps = P['MCF_MAX_NUM_MISSES'] + 1
    D = np.arange(0, max_px + 1)
    table = np.empty((gaps, max_px + 1))
    dmax = np.zeros(gaps, np.int32)
    for g in range(1, gaps + 1):
        distances = ((D / max_px) - 1) * -1
        with np.errstate(divide='ignore'):
            costs = -np.log((1 - w) * distances * (P['MCF_MISS_RATE'] ** (g - 1)) + w * vis_sim + 1e-6)
        costs[distances == 0] = np.inf
        table[g - 1] = costs
        ok = np.nonzero(costs[1:] < P['MCF_EDGE_COST_THR'])[0]
        dmax[g - 1] = ok.max() + 1 if len(ok) else 0
    return table, dmax


class AxonDetections(object):
    def __init__(self, model, dataset, parameters, directory, timepoint_subset=None):
        self.model = model
        self.dataset = dataset
        self.name = dataset.name
        self.dir = directory
        if self.dir:
            os.makedirs(self.dir, exist_ok=True)
        # AxonDetections.py:52-55: the detection frames to work on (default: all). Detection, association and every
        # per-frame accessor then index POSITIONS in this list, as the reference's do (its loops run over
        # range(len(self)) and look frames up through timepoint_subset).
        if timepoint_subset is None:
            self.timepoint_subset = range(self.dataset.sizet)      # (kept as a range: nothing per frame on the way to the first launch)
        else:
            self.timepoint_subset = [int(t) for t in timepoint_subset]
            if any(t < 0 or t >= self.dataset.sizet for t in self.timepoint_subset):
                raise ValueError(f'timepoint_subset must lie in [0, {self.dataset.sizet})')
        self.P = dict(parameters)
        self.device = dataset.device
        self.Sx, self.Sy, self.tilesize = parameters['SX'], parameters['SY'], parameters['TILESIZE']
        if (self.Sx, self.Sy, self.tilesize) != (hp.S, hp.S, hp.TILE):
            raise ValueError('the HIP detector is specialised for TILESIZE=512, SX=SY=12')
        self.nms_min_dist = parameters.get('NON_MAX_SUPRESSION_DIST')
        self.conf_thr = parameters['BBOX_THRESHOLD']
        self.all_conf_thrs = _conf_thresholds(self.conf_thr)
        self.max_px_assoc_dist = hp.MAX_PX_ASSOC_DIST
        self.axon_box_size = hp.AXON_BOX_SIZE
        self.labelled = False
        self.conn8 = bool(parameters.get('ASTAR_8_CONNECTED', False))
        self.reproduce_label_quirk = bool(parameters.get('REPRODUCE_FRAME_LABEL_QUIRK', True))
        # Every attribute the class reads is created here, at its empty value. The cached ones form two groups with one
        # reset point each -- whoever adds a cached attribute adds it to one of the two methods, and by that to __init__.
        self.d_conf = self.d_x = self.d_y = self.d_count = None
        self._drop_detections()
        # state that follows neither the detections nor the association: the labels, the target and its fields
        self._gt = self._gt_ids = self._gt_dev = self._gt_gid_dev = None
        self._gt_no = 0
        self._target_cells, self.reach_px, self.structure_outputchannel_coo, self._target_fields = None, None, None, {}
        if getattr(dataset, 'labelled', False):            # a labelled dataset brings its ground truth (AxonDetections.py:57)
            self.set_groundtruth([dataset.labels[t] for t in self.timepoint_subset])

    def _drop_association(self):
        """Forget everything that belongs to one association (assign_ids / _set_ided_from_tables)."""
        self._solved = False
        self._d_track, self._track_flat_cache = None, None
        self._n_ids, self._n_tracks_dev = None, None
        self.mcf_total_cost, self.mcf_certificate = None, None
        self._ided_tables, self.IDed_dets_all, self.IDed_dets_block = None, None, None
        self._recon = None

    def _drop_detections(self, keep_grids=False):
        """Forget everything that belongs to one set of detection arrays (d_conf, d_x, d_y, d_count), the association
        included. keep_grids: the YOLO grids the arrays were decoded from stay (gather_detections: this rank's own)."""
        self._host, self._det_tables = None, None
        self._hist, self._shard = None, None
        self._target_dets, self._target_path_cache = None, None
        if not keep_grids:
            self._yolo, self.tile_yx, self._tiled_tables = None, None, None
        self._drop_association()

    @property
    def n_ids(self):
        """Number of identities of the last association (None: adopted from a cache, ids are whatever the cache holds). The
        frame-to-frame variant leaves the count on the device; it is fetched when somebody asks."""
        if self._n_ids is None and self._n_tracks_dev is not None:
            self._n_ids = int(self._n_tracks_dev.item())
        return self._n_ids

    @n_ids.setter
    def n_ids(self, value):
        self._n_ids, self._n_tracks_dev = value, None

    def __len__(self):
        """Number of detection frames (after a multi-GPU gather: of the whole timelapse)."""
        return int(self.d_count.shape[0]) if self.d_count is not None else len(self.timepoint_subset)

    # ------------------------------------------------------------------ caches (AxonDetections.py:141-176)
    def _cache_fname(self, which):
        return f'{self.dir}/{self.dataset.name}_{which}.pkl'

    def from_cache(self, which):
        with open(self._cache_fname(which), 'rb') as file:
            return pickle.load(file)

    def to_cache(self, which, dat):
        with open(self._cache_fname(which), 'wb') as file:
            pickle.dump(dat, file)

    # ------------------------------------------------------------------ detection (AxonDetections.py:87-139)
    def detect_dataset(self, cache=None):
        if cache == 'from':
            self._set_detections_from_tables(self.from_cache('_detections'))
            return
        frames = self.dataset.frames
        if hasattr(self.model, 'set_arith'):
            self.model.set_arith(self.P.get('CNN_ARITH', 'f32'))       # read at inference time, like every parameter
        streamed = self._detect_streaming() if getattr(self.dataset, '_pending', False) else None
        self._drop_detections()
        self.tile_yx = self.dataset.tile_yx
        if not self.tile_yx:
            raise ValueError('the timelapse is empty (no tile has a non-zero pixel)')
        # the frames of timepoint_subset (AxonDetections.py:111), one launch sequence per run of consecutive frames
        sub = self.timepoint_subset
        whole = isinstance(sub, range)
        runs, a = [], 0
        if whole:
            runs = [(0, len(sub))]
        else:
            for k in range(1, len(sub) + 1):
                if k == len(sub) or sub[k] != sub[k - 1] + 1:
                    runs.append((sub[a], k - a))
                    a = k
        if streamed is not None and streamed[0] == self.tile_yx and whole:
            self._yolo = streamed[1]                                 # computed chunk by chunk beside the copies
        else:
            parts = [self.model.detect_frames(frames, self.tile_yx, t0, n) for t0, n in runs]
            self._yolo = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
        thr = float(np.float32(self.all_conf_thrs.min()))
        self.d_conf, self.d_x, self.d_y, self.d_count = hp.decode_stitch_nms(
            self._yolo, self.tile_yx, thr, self.nms_min_dist)
        import torch.distributed as dist
        if self.d_conf.shape[1] > 2048 and not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            # large frames (more than 14 tiles): the arrays were sized for one detection per grid cell; keep what the fullest
            # frame needs (the arc builder's scratch and the frame-to-frame variant scale with the capacity). Frame-sharded
            # ranks agree on a common capacity in gather_detections().
            self._shrink_capacity(int(self.d_count.max().item()))
        if cache == 'to':
            self.to_cache('_detections', self._detections)

    def _detect_streaming(self):
        """Host-resident input (Timelapse.from_host_u16): the CNN of the detection frames every chunk completes is
        enqueued right behind the chunk's preprocessing, while the next chunk's H2D copy runs on the copy stream. The
        kept-tile list is a property of the whole timelapse (Timelapse.py:551-558) and only known after the last chunk:
        the chunks are detected with every tile, which is the final list unless some tile is empty at EVERY time point
        (then detect_dataset repeats the detection on the resident frames with the right list). Returns (tile list used,
        YOLO grids [sizet, n_tiles, 12,12,3])."""
        ds = self.dataset
        tiles = [(ty, tx) for ty in range(ds.ytiles) for tx in range(ds.xtiles)]
        ctx = ds.temporal_context
        # the front of the network (conv blocks 0-5: 87 % of the FLOPs) chunk by chunk, the rest once for all frames: the first
        # linear layer streams its 168 MB of weights per call, whatever the batch
        split = ds.sizet * len(tiles) <= getattr(self.model, 'max_batch', 0)
        parts, done, occ = [], 0, None
        for a, b, occ in ds.stream_chunks():
            ready = min(max(b - 2 * ctx, 0), ds.sizet)               # detection frame t reads input frames t .. t + 2 ctx
            if ready > done:
                if split:
                    self.model.front_frames(ds.frames, tiles, done, ready - done, done * len(tiles))
                else:
                    parts.append(self.model.detect_frames(ds.frames, tiles, done, ready - done))
                done = ready
        yolo = self.model.back(ds.sizet, len(tiles)) if split else (parts[0] if len(parts) == 1 else torch.cat(parts, 0))
        ds._occ_done.synchronize()                                    # (a few bytes, behind the last chunk's preprocessing)
        ds._tile_yx = hp.tile_list(ds._occ_host, ds.sizey, ds.sizex)
        return tiles, yolo

    def _shrink_capacity(self, fullest):
        cap = min(-(-max(int(fullest), 1) // 64) * 64, int(self.d_conf.shape[1]))
        self.d_conf, self.d_x, self.d_y = (a[:, :cap].contiguous() for a in (self.d_conf, self.d_x, self.d_y))
        # gather_detections() can get here with caches filled (tables or histograms read after detect_dataset()): they have
        # the old capacity. In detect_dataset() everything was dropped a few lines earlier.
        self._drop_detections(keep_grids=True)

    def gather_detections(self, group=None):
        """Frame-sharded runs: every rank has detected its own contiguous block of frames; one
        all-gather (RCCL over xGMI on GPUs) gives every rank the detections of the whole
        timelapse, in rank order, before the global flow solve. Blocks must have equal length."""
        from .sharded import all_gather_detections
        import torch.distributed as dist
        local = int(self.d_count.shape[0])
        if self.d_conf.shape[1] > 2048 and dist.is_initialized() and dist.get_world_size(group) > 1:
            # large frames: every rank keeps what the fullest frame of the WHOLE timelapse needs (one MAX all-reduce over
            # the group of the gather), so that the gathered arrays fit the association kernels' capacity
            from .sharded import _collective
            fullest = self.d_count.max().reshape(1).clone()
            _collective('capacity_allreduce', lambda: dist.all_reduce(fullest, op=dist.ReduceOp.MAX, group=group))
            self._shrink_capacity(int(fullest.item()))
        gathered_hist = None
        if self.P['MCF_VIS_SIM_WEIGHT'] and dist.is_initialized() and dist.get_world_size(group) > 1:
            # the appearance features need the pixels, which only the owning rank has: they travel with the detections
            hist, hsum = self._appearance()               # (of the local arrays: before they are replaced)
            world = dist.get_world_size(group)
            g_hist = torch.empty((world * local,) + tuple(hist.shape[1:]), dtype=hist.dtype, device=hist.device)
            g_hsum = torch.empty((world * local, hsum.shape[1]), dtype=hsum.dtype, device=hsum.device)
            dist.all_gather_into_tensor(g_hist, hist.contiguous(), group=group)
            dist.all_gather_into_tensor(g_hsum, hsum.contiguous(), group=group)
            gathered_hist = (g_hist, g_hsum)
        self._drop_detections(keep_grids=True)
        self.d_conf, self.d_x, self.d_y, self.d_count = all_gather_detections(
            self.d_conf, self.d_x, self.d_y, self.d_count, group,
            check_shapes=not getattr(self.dataset, '_gather_shapes_agree', False))
        self.dataset._gather_shapes_agree = True          # the shapes follow from the timelapse: checked once
        self._hist = gathered_hist
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            r = dist.get_rank(group)
            self._shard = (r * local, (r + 1) * local, group)       # this rank's frames within the gathered arrays

    def set_detections(self, conf, x, y, count):
        """Adopt detection lists that are already arrays (conf f32 [F,cap], x / y i32 [F,cap], count i32 [F], every frame
        in descending confidence): association-only workloads (bench.py --workload assoc-*) and detections produced
        elsewhere. The arrays go to the dataset's device; detect_dataset() is not needed afterwards."""
        self._drop_detections()
        dev = self.device
        as_dev = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
        self.d_conf, self.d_x, self.d_y, self.d_count = (as_dev(conf, torch.float32), as_dev(x, torch.int32), as_dev(y, torch.int32),
                                                         as_dev(count, torch.int32))
        if self.d_conf.dim() != 2 or self.d_x.shape != self.d_conf.shape or self.d_y.shape != self.d_conf.shape \
                or self.d_count.shape != (self.d_conf.shape[0],):
            raise ValueError('conf, x, y must be [F, cap] and count [F]')

    def _host_dets(self):
        """(count i32 [F], conf f32 [F,cap], x, y) on the host, fetched once."""
        if self._host is None:
            self._host = (self.d_count.cpu().numpy(), self.d_conf.cpu().numpy(), self.d_x.cpu().numpy(),
                          self.d_y.cpu().numpy())
        return self._host

    def _set_detections_from_tables(self, tables):
        F = len(tables)
        cap = max([len(t) for t in tables] + [1])
        conf = np.zeros((F, cap), np.float32); x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
        cnt = np.zeros(F, np.int32)
        for f, t in enumerate(tables):
            n = len(t)
            cnt[f] = n
            conf[f, :n] = t.conf.to_numpy(dtype=np.float32)
            x[f, :n] = t.anchor_x.to_numpy(dtype=np.int32)
            y[f, :n] = t.anchor_y.to_numpy(dtype=np.int32)
        self._drop_detections()
        self.d_conf, self.d_x, self.d_y, self.d_count = (torch.from_numpy(a).to(self.device) for a in (conf, x, y, cnt))
        self._host, self._det_tables = (cnt, conf, x, y), list(tables)

    @property
    def _detections(self):
        """list of per-frame DataFrames [conf Float32, anchor_x Int64, anchor_y Int64], index
        Axon_000.. in descending confidence (AxonDetections.py:235,261,276-277)."""
        if self._det_tables is None:
            cnt, conf, x, y = self._host_dets()
            tabs = []
            for f in range(len(cnt)):
                n = int(cnt[f])
                tabs.append(pd.DataFrame({'conf': pd.array(conf[f, :n], dtype='Float32'),
                                          'anchor_x': pd.array(x[f, :n].astype(np.int64), dtype='Int64'),
                                          'anchor_y': pd.array(y[f, :n].astype(np.int64), dtype='Int64')},
                                         index=[f'Axon_{i:0>3}' for i in range(n)]))
            self._det_tables = tabs
        return self._det_tables

    @property
    def _pandas_tiled_dets(self):
        """_yolo_Y2pandas_det (AxonDetections.py:178-248) of every frame: per frame a list over the kept tiles of tables
        [conf Float32, anchor_x Int64, anchor_y Int64] in TILE coordinates, the cells at or above the confidence floor
        named Axon_000.. in cell order and sorted by ascending confidence -- the tables before stitching and NMS. The
        hot path never needs them (its kernel goes from the YOLO grids to the frame's final list), so they are decoded
        from the grids on the host when first asked for: f32 arithmetic, half-to-even rounding, all-zero cells left
        at zero, exactly as :192-210."""
        if self._tiled_tables is None:
            if self._yolo is None:
                raise ValueError('the tile tables come from the YOLO grids: run detect_dataset() (not from a cache)')
            y = self._yolo.cpu().numpy().astype(np.float32, copy=False)            # [F, n_tiles, Sx, Sy, 3]
            ii = np.arange(self.Sx, dtype=np.float32).reshape(1, 1, self.Sx, 1)
            jj = np.arange(self.Sy, dtype=np.float32).reshape(1, 1, 1, self.Sy)
            ts = np.float32(self.tilesize)
            ax = np.rint(((y[..., 1] + ii) * ts) / np.float32(self.Sx))
            ay = np.rint(((y[..., 2] + jj) * ts) / np.float32(self.Sy))
            zero = (y == 0).all(-1)
            ax[zero] = 0
            ay[zero] = 0
            thr = np.float32(self.all_conf_thrs.min())
            frames = []
            for f in range(y.shape[0]):
                tiles = []
                for k in range(y.shape[1]):
                    conf = y[f, k, ..., 0].reshape(-1)
                    keep = np.nonzero(conf >= thr)[0]
                    order = keep[np.argsort(conf[keep], kind='stable')]       # ties stay in cell order
                    names = np.empty(len(conf), dtype=object)
                    names[keep] = [f'Axon_{i:0>3}' for i in range(len(keep))]
                    tiles.append(pd.DataFrame({'conf': pd.array(conf[order], dtype='Float32'),
                                               'anchor_x': pd.array(ax[f, k].reshape(-1)[order].astype(np.int64), dtype='Int64'),
                                               'anchor_y': pd.array(ay[f, k].reshape(-1)[order].astype(np.int64), dtype='Int64')},
                                              index=list(names[order])))
                frames.append(tiles)
            self._tiled_tables = frames
        return self._tiled_tables

    # ------------------------------------------------------------------ access (AxonDetections.py:280-353)
    def get_frame_dets(self, which_dets, t, libmot=False, unstitched=False):
        if t is None:
            all_dets = [self.get_frame_dets(which_dets, t, libmot) for t in range(len(self))]
            return pd.concat(all_dets, axis=not libmot)
        if unstitched:
            # only for 'all' and 'confident' (AxonDetections.py:322-331): the tile-wise list of tables
            if which_dets == 'all':
                return [d.copy() for d in self._pandas_tiled_dets[t]]
            if which_dets == 'confident':
                return [d[d.conf > self.conf_thr] for d in self._pandas_tiled_dets[t]]
            raise ValueError("unstitched=True goes with which_dets 'all' or 'confident'")
        if which_dets == 'all':
            det = self._detections[t]
        elif which_dets == 'confident':
            det = self._detections[t][self._detections[t].conf > self.conf_thr]
        elif which_dets == 'IDed':
            assert self._IDed_detections, "Run .assign_IDs() first!"
            det = self._IDed_detections[t]
        elif which_dets == 'groundtruth':
            if not self.labelled:
                raise ValueError("no labels: call set_groundtruth() first")
            gx, gy = self._gt[t]
            det = pd.DataFrame({'conf': pd.array(np.ones(len(gx), np.float32), dtype='Float32'),
                                'anchor_x': pd.array(np.asarray(gx, np.int64), dtype='Int64'),
                                'anchor_y': pd.array(np.asarray(gy, np.int64), dtype='Int64')},
                               index=[f'Axon_{i:0>3}' for i in self._gt_ids[t]])
        elif which_dets == 'FP_FN':
            # AxonDetections.py:341-349: the confident detections that match no label, the labels no detection matches
            if not self.labelled:
                raise ValueError("no labels: call set_groundtruth() first")
            FP_mask, FN_mask = self.compute_TP_FP_FN('confident', t, return_FP_FN_mask=True)
            return self.get_frame_dets('confident', t)[FP_mask], self.get_frame_dets('groundtruth', t)[FN_mask]
        else:
            raise NotImplementedError(f"which_dets={which_dets!r} is a plotting selection (out of scope)")
        if libmot:
            return self.det2libmot_det(det, t)
        return det.copy()

    def det2libmot_det(self, detection, t):
        """AxonDetections.py:754-784"""
        conf, x, y = detection.values.T
        half = self.axon_box_size // 2
        frame_id = np.full(conf.shape, t)
        boxs = np.full(conf.shape, self.axon_box_size)
        # the reference takes idx[-3:], which folds identities >= 1000 onto 0..999; the whole number is used here
        axon_id = np.array([_axon_number(idx) for idx in detection.index])
        det_libmot = np.stack([frame_id, axon_id, x - half, y - half, boxs, boxs, conf]).T
        cols = ['FrameId', 'Id', 'X', 'Y', 'Width', 'Height', 'conf']
        return pd.DataFrame(det_libmot, columns=cols).set_index(['FrameId', 'Id'])

    # ------------------------------------------------------------------ detection metrics (AxonDetections.py:378-503)
    def set_groundtruth(self, labels):
        """labels: per detection frame (x, y) or (x, y, ids) -- integer anchor arrays and, for the tracking scores of
        search_MCF_params, the axons' identities (the numbers of the labels' Axon_### names; default: position in
        the frame). The reference reads them from the labelled dataset's YOLO targets (get_frame_and_truedets,
        :355-376); here a labelled Timelapse (prepare_training_data) hands its labels over in __init__."""
        if len(labels) != len(self):
            raise ValueError(f'{len(labels)} label frames for {len(self)} detection frames')
        self._gt = [(np.asarray(l[0], np.int64), np.asarray(l[1], np.int64)) for l in labels]
        self._gt_ids = [np.asarray(l[2], np.int64) if len(l) > 2 else np.arange(len(l[0])) for l in labels]
        if any(len(i) != len(x) or len(np.unique(i)) != len(i) for i, (x, _) in zip(self._gt_ids, self._gt)):
            raise ValueError('label identities must be unique within a frame and match the anchors in number')
        gcap = max([len(x) for x, _ in self._gt] + [1])
        gx = np.zeros((len(self), gcap), np.int32); gy = np.zeros((len(self), gcap), np.int32)
        for t, (x, y) in enumerate(self._gt):
            gx[t, :len(x)] = x; gy[t, :len(y)] = y
        dev = self.device
        self._gt_dev = (torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev),
                        torch.tensor([len(x) for x, _ in self._gt], dtype=torch.int32, device=dev))
        # the dense label identities (rank among all identities of the labels) for the tracking scores on the device
        every = np.unique(np.concatenate(self._gt_ids + [np.zeros(0, np.int64)]))
        gid = np.zeros((len(self), gcap), np.int32)
        for t, ids in enumerate(self._gt_ids):
            gid[t, :len(ids)] = np.searchsorted(every, ids)
        self._gt_gid_dev, self._gt_no = torch.from_numpy(gid).to(dev), len(every)
        self.labelled = True

    def detection_confusion(self):
        """compute_TP_FP_FN('all', t) of every frame in one launch: int array [frames, 3 (TP, FP, FN), 13 thresholds]."""
        if not self.labelled:
            raise ValueError("no labels: call set_groundtruth() first")
        return hp.detection_confusion(self.d_conf, self.d_x, self.d_y, self.d_count, *self._gt_dev, self.all_conf_thrs,
                                      self.nms_min_dist).cpu().numpy().astype(np.int64)

    def compute_TP_FP_FN(self, which_dets, t, return_FP_FN_mask=False):
        """AxonDetections.py:409-466 for one frame and one selection of detections ('all', 'confident', 'IDed')."""
        det = self.get_frame_dets(which_dets, t)
        dev = self.device
        n = len(det)
        conf = torch.zeros((1, max(n, 1)), dtype=torch.float32, device=dev)
        x = torch.zeros((1, max(n, 1)), dtype=torch.int32, device=dev); y = torch.zeros_like(x)
        if n:
            conf[0, :n] = torch.from_numpy(det.conf.to_numpy(dtype=np.float32))
            x[0, :n] = torch.from_numpy(det.anchor_x.to_numpy(dtype=np.int32))
            y[0, :n] = torch.from_numpy(det.anchor_y.to_numpy(dtype=np.int32))
        cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        gx, gy, gc = (v[t:t + 1].contiguous() for v in self._gt_dev)
        k = int(np.where(self.all_conf_thrs == self.conf_thr)[0][0]) if return_FP_FN_mask else -1
        res = hp.detection_confusion(conf, x, y, cnt, gx, gy, gc, self.all_conf_thrs, self.nms_min_dist, k)
        if return_FP_FN_mask:
            _, fp, fn = res
            return fp[0, :n].cpu().numpy().astype(bool), fn[0, :int(gc.item())].cpu().numpy().astype(bool)
        return res[0].cpu().numpy().astype(np.int64)

    def compute_prc_rcl_F1(self, cnfs_mtrx, return_dataframe=False):
        """AxonDetections.py:468-503 (host arithmetic, three lines)."""
        prc = cnfs_mtrx[0] / (cnfs_mtrx[0] + cnfs_mtrx[1] + 1e-6)
        rcl = cnfs_mtrx[0] / (cnfs_mtrx[0] + cnfs_mtrx[2] + 1e-6)
        f1 = 2 * (prc * rcl) / ((prc + rcl) + 1e-6)
        metric = np.array([prc, rcl, f1]).round(3)
        if return_dataframe:
            index = pd.MultiIndex.from_product([('precision', 'recall', 'F1'), self.all_conf_thrs])
            return pd.Series(metric.flatten(), index=index)
        return metric

    def get_detection_metrics(self, which_dets, t, return_all_conf_thrs=False):
        """AxonDetections.py:378-407"""
        if not self.labelled:
            return None, None, None
        prc_rcl_f1 = self.compute_prc_rcl_F1(self.compute_TP_FP_FN(which_dets, t))
        if not return_all_conf_thrs:
            return prc_rcl_f1[:, np.where(self.all_conf_thrs == self.conf_thr)[0][0]]
        return prc_rcl_f1

    # ------------------------------------------------------------------ association (AxonDetections.py:505-524)
    def assign_ids(self, astar_paths_cache=None, assigedIDs_cache=None, _len_table=None):
        """AxonDetections.py:505-524. astar_paths_cache: 'from' adopts the path lengths of a
        '{name}_astar_dets_paths.pkl' (the reference's format: per frame pair a nested list of coo matrices / None)
        instead of computing them; 'to' writes such a file (astar_dets_paths)."""
        self._drop_association()
        if assigedIDs_cache == 'from':
            self._set_ided_from_tables(self.from_cache('_IDed_detections'))
        else:
            if astar_paths_cache == 'from':
                _len_table = self._length_table_from_paths(self.from_cache('astar_dets_paths'))
            elif astar_paths_cache == 'to':
                self.to_cache('astar_dets_paths', self.astar_dets_paths())
            self._solved = self._assign_IDs_to_detections(_len_table)
            if assigedIDs_cache == 'to' and self._solved:
                self.to_cache('_IDed_detections', self._IDed_detections)
        self.IDed_dets_all = self._agg_all_IDed_dets() if self._solved else None

    @property
    def _IDed_detections(self):
        """list of per-frame DataFrames of the IDed detections, rows sorted by ID, index Axon_{id:03}
        (libmot_det2det, AxonDetections.py:786-823); None if the flow problem was infeasible (:691-696).
        Built on first access -- the hot path itself only keeps arrays."""
        if not self._solved:
            return None
        if self._ided_tables is None:
            cnt, conf, x, y = self._host_dets()
            frame, tid, c, xx, yy = self.ided_arrays()
            order = np.lexsort((tid, frame))
            frame, tid, c, xx, yy = frame[order], tid[order], c[order], xx[order], yy[order]
            bounds = np.searchsorted(frame, np.arange(len(cnt) + 1))
            tabs = []
            for f in range(len(cnt)):
                lo, hi = bounds[f], bounds[f + 1]
                if lo == hi:
                    tabs.append(pd.DataFrame([]))          # "if frame empty, no detections" (:819-821)
                    continue
                tabs.append(pd.DataFrame({'conf': pd.array(c[lo:hi], dtype='Float32'),
                                          'anchor_x': pd.array(xx[lo:hi].astype(np.int64), dtype='Int64'),
                                          'anchor_y': pd.array(yy[lo:hi].astype(np.int64), dtype='Int64')},
                                         index=[f'Axon_{i:0>3}' for i in tid[lo:hi]]))
            self._ided_tables = tabs
        return self._ided_tables

    def _set_ided_from_tables(self, tables):
        """Adopt reference-format per-frame IDed tables (the '_IDed_detections' cache)."""
        self._drop_association()
        cnt, conf, x, y = self._host_dets()
        offs = self._offs
        track = np.full(int(offs[-1]), -1, np.int32)
        for f, t in enumerate(tables):
            if len(t) == 0:
                continue
            tx, ty = t.anchor_x.to_numpy(dtype=np.int64), t.anchor_y.to_numpy(dtype=np.int64)
            for name, ax, ay in zip(t.index, tx, ty):
                k = np.nonzero((x[f, :cnt[f]] == ax) & (y[f, :cnt[f]] == ay))[0][0]   # exact anchor match (:804-808)
                track[offs[f] + k] = _axon_number(name)
        self._track_flat_cache = track                              # (n_ids stays None: ids are whatever the cache holds)
        self._solved, self._ided_tables = True, list(tables)

    def _frame_pairs(self):
        """(t, t_bef, label) of every frame pair the tracker may link: t_bef = t-1 .. t-(MCF_MAX_NUM_MISSES+1), not before
        frame 0, in the order and with the labels of the reference's loops (AxonDetections.py:544-556) -- the order of the
        'astar_dets_paths' cache's dictionary."""
        gaps = self.P['MCF_MAX_NUM_MISSES'] + 1
        for t in range(len(self)):
            for t_bef in range(t - 1, max(t - gaps, 0) - 1, -1):
                yield t, t_bef, f'{self.dataset.name}_t:{t:0>3}-t:{t_bef:0>3}'

    def astar_dists(self):
        """_get_astar_path_distances(_compute_detections_astar_paths()) (AxonDetections.py:526-585,717-752):
        dict '{name}_t:{t:03}-t:{t_bef:03}' -> int array [N_t_bef, N_t], computed on the GPU per pair."""
        cnt = self._host_dets()[0]
        out = {}
        for t, t_bef, lbl in self._frame_pairs():
            na, nb = int(cnt[t_bef]), int(cnt[t])
            if na == 0:
                out[lbl] = np.array([])
                continue
            D = hp.path_cost(self.d_x[t_bef, :na], self.d_y[t_bef, :na], self.d_x[t, :nb], self.d_y[t, :nb],
                             self.dataset.sizey, self.dataset.sizex, self._mask_dev(t),      # _get_maskweights(t), AxonDetections.py:557
                             self.max_px_assoc_dist, self.conn8)
            out[lbl] = D.cpu().numpy()
        return out

    def _length_table_from_dists(self, dists):
        """astar_dists() (int matrices per frame pair, max_px_assoc_dist = none) as the i16 table [F, cap, gaps, cap]
        the arc builder reads (0 = none)."""
        F, cap, gaps = len(self), self.d_x.shape[1], self.P['MCF_MAX_NUM_MISSES'] + 1
        table = np.zeros((F, cap, gaps, cap), np.int16)
        for t, t_bef, lbl in self._frame_pairs():
            D = dists[lbl]
            if D.ndim == 2 and D.size:
                table[t_bef, :D.shape[0], t - t_bef - 1, :D.shape[1]] = np.where(D >= self.max_px_assoc_dist, 0, D)
        return torch.from_numpy(table).to(self.device)

    def _length_table_from_paths(self, paths):
        """_get_astar_path_distances (AxonDetections.py:717-752) of a cached path dictionary, as the i16 table
        [F, cap, gaps, cap] axt_build_arcs reads as d_len_table: getnnz() of a path, 0 (= none) for None."""
        cnt = self._host_dets()[0]
        F, cap, gaps = len(self), self.d_x.shape[1], self.P['MCF_MAX_NUM_MISSES'] + 1
        table = np.zeros((F, cap, gaps, cap), np.int16)
        for t, t_bef, lbl in self._frame_pairs():
            rows = paths[lbl]
            if len(rows) != cnt[t_bef] or any(len(r) != cnt[t] for r in rows):
                raise ValueError(f'cached paths of t:{t}-t:{t_bef} do not match the detections')
            for i, row in enumerate(rows):
                table[t_bef, i, t - t_bef - 1, :len(row)] = [0 if p is None else min(p.getnnz(), 32767) for p in row]
        return torch.from_numpy(table).to(self.device)

    def astar_dets_paths(self):
        """The reference's path dictionary (_compute_detections_astar_paths, AxonDetections.py:526-585): per frame pair
        a list over the detections of t_bef of lists over the detections of t of scipy coo matrices [H, W] (bool)
        marking the cells of a shortest path, or None beyond max_px_assoc_dist. On an all-ones mask every monotone
        staircase between the two anchors is a shortest path; this one walks the columns first, then the rows
        (8-connected: the diagonal first, then straight) (which
        of the equally short paths pyastar2d returns is unpinned; lengths are what the tracker
        uses). On a masked grid the GPU search walks back from every target along its distance field
        (axt_path_cells)."""
        if self.dataset.masked:
            return self._masked_dets_paths()
        return self._open_dets_paths(self.astar_dists())

    def _open_dets_paths(self, dists):
        """The paths of frame pairs on an all-ones mask (closed form): dists = {label: length matrix} of those pairs."""
        from scipy import sparse
        cnt, _, x, y = self._host_dets()
        H, W = self.dataset.sizey, self.dataset.sizex
        out = {}
        for lbl, D in dists.items():
            t, t_bef = (int(v) for v in re.search(r't:(\d+)-t:(\d+)$', lbl).groups())
            rows = []
            for i in range(int(cnt[t_bef])):
                row = []
                for j in range(int(cnt[t])):
                    if D[i, j] >= self.max_px_assoc_dist:
                        row.append(None)
                        continue
                    xa, ya, xb, yb = int(x[t_bef, i]), int(y[t_bef, i]), int(x[t, j]), int(y[t, j])
                    sx, sy = (1 if xb >= xa else -1), (1 if yb >= ya else -1)
                    if self.conn8:                      # diagonal first, then straight: max(|dx|,|dy|) + 1 cells
                        k = min(abs(xb - xa), abs(yb - ya))
                        dx, dy = abs(xb - xa) - k, abs(yb - ya) - k
                        c = np.concatenate([xa + sx * np.arange(k + 1), xa + sx * (k + np.arange(1, dx + 1)),
                                            np.full(dy, xb)]).astype(np.int64)
                        r = np.concatenate([ya + sy * np.arange(k + 1), np.full(dx, ya + sy * k),
                                            ya + sy * (k + np.arange(1, dy + 1))]).astype(np.int64)
                    else:
                        xs = np.arange(xa, xb + sx, sx)
                        ys = np.arange(ya, yb + sy, sy)
                        r = np.concatenate([np.full(len(xs), ya), ys[1:]])
                        c = np.concatenate([xs, np.full(len(ys) - 1, xb)])
                    row.append(sparse.coo_matrix((np.ones(len(r)), (r, c)), (H, W), bool))
                rows.append(row)
            out[lbl] = rows
        return out

    def _masked_dets_paths(self):
        """astar_dets_paths on a masked grid: one exact single-source search per detection of t_bef, then the walk
        back from every detection of t (hotpath.path_cells)."""
        from scipy import sparse
        cnt = self._host_dets()[0]
        H, W = self.dataset.sizey, self.dataset.sizex
        out = {}
        for t, t_bef, lbl in self._frame_pairs():
            grid = self._mask_dev(t)
            na, nb = int(cnt[t_bef]), int(cnt[t])
            if na == 0 or nb == 0:
                out[lbl] = [[] for _ in range(na)]
                continue
            if grid is None:
                # a frame of a time-varying mask that is all ones: the closed-form staircase of the open grid
                D = hp.path_cost(self.d_x[t_bef, :na], self.d_y[t_bef, :na], self.d_x[t, :nb], self.d_y[t, :nb],
                                 H, W, None, self.max_px_assoc_dist, self.conn8).cpu().numpy()
                out.update(self._open_dets_paths({lbl: D}))
                continue
            D, cells = hp.path_cells(self.d_x[t_bef, :na], self.d_y[t_bef, :na], self.d_x[t, :nb], self.d_y[t, :nb],
                                     H, W, grid, self.max_px_assoc_dist, self.conn8)
            D, cells = D.cpu().numpy(), cells.cpu().numpy()
            coo = lambda c: sparse.coo_matrix((np.ones(len(c)), (c // W, c % W)), (H, W), bool)
            out[lbl] = [[None if D[i, j] >= self.max_px_assoc_dist else coo(cells[i, j, :D[i, j]]) for j in range(nb)]
                        for i in range(na)]
        return out

    def search_MCF_params(self, edge_cost_thr_values=(.4, .6, .7, .8, .9, 1, 1.2, 3),
                          entry_exit_cost_values=(.2, .8, .9, 1, 1.1, 2), miss_rate_values=(0.9, 0.6),
                          vis_sim_weight_values=(0, 0.1), conf_capping_method_values=('ceil', 'scale_to_max'),
                          scoring='host', score_batch=64):
        """AxonDetections.py:845-922: re-solve the association for every combination of the five tracker parameters
        (same nesting order) and score each against the labelled identities; one row per combination -- the five
        parameters, then mot_metrics.MOTCHALLENGE_METRICS -- written to '{dir}/MCF_params_results.csv' and returned.
        Every solve is the GPU arc build + flow solve of assign_ids (the detections and their appearance
        histograms stay on the device between combinations); the parameters are restored afterwards. On a masked
        grid the path lengths are computed once, exactly and up to max_px_assoc_dist (astar_dists), and reused by every
        combination -- as the reference reuses its path cache.
        scoring: 'host' scores every combination with mot_metrics on the libmot tables; 'gpu' keeps every combination's
        track table on the device and scores score_batch of them per call of score_associations --
        same rows, columns and CSV."""
        from . import mot_metrics
        if not self.labelled:
            raise ValueError("no labels: call set_groundtruth() first")
        if scoring not in ('host', 'gpu'):
            raise ValueError(f"scoring={scoring!r}: 'host' or 'gpu'")
        if scoring == 'gpu':
            return self._search_MCF_params_gpu(edge_cost_thr_values, entry_exit_cost_values, miss_rate_values,
                                               vis_sim_weight_values, conf_capping_method_values, int(score_batch))
        target = self.get_frame_dets('groundtruth', None, libmot=True)
        names = ('edge_cost_thr', 'entry_exit_cost', 'miss_rate', 'vis_sim_weight', 'conf_capping_method')
        keys = ('MCF_EDGE_COST_THR', 'MCF_ENTRY_EXIT_COST', 'MCF_MISS_RATE', 'MCF_VIS_SIM_WEIGHT', 'MCF_CONF_CAPPING_METHOD')
        before = {k: self.P[k] for k in keys}
        results = []
        # masked grid: the exact path lengths once, for every threshold of the grid (the reference reads its path cache
        # in every iteration, :882); all-ones masks have closed-form lengths
        lengths = self._length_table_from_dists(self.astar_dists()) if self.dataset.masked else None
        try:
            for ec in edge_cost_thr_values:
                for eec in entry_exit_cost_values:
                    for mr in miss_rate_values:
                        for vsw in vis_sim_weight_values:
                            for ccm in conf_capping_method_values:
                                self.P.update(dict(zip(keys, (ec, eec, mr, vsw, ccm))))
                                self.assign_ids(_len_table=lengths)
                                pred = self.get_frame_dets('IDed', None, libmot=True) if self._solved else None
                                ev = mot_metrics.compare_to_groundtruth(target, pred, float(self.nms_min_dist) ** 2)
                                results.append(pd.concat([pd.Series((ec, eec, mr, vsw, ccm), names, dtype=object),
                                                          mot_metrics.summarize(ev)]))
        finally:
            self.P.update(before)
        results = pd.concat(results, axis=1).T
        os.makedirs(self.dir, exist_ok=True)
        results.to_csv(f'{self.dir}/MCF_params_results.csv')
        return results

    def _search_MCF_params_gpu(self, ecs, eecs, mrs, vsws, ccms, score_batch):
        """search_MCF_params with the scores taken on the device: the same loop, but every combination leaves a clone of
        its track table (all -1 where nothing was solved: the host path's pred = None) and the tables are scored
        score_batch at a time."""
        if score_batch < 1:
            raise ValueError(f'score_batch={score_batch} must be positive')
        self._require_scorable()
        names = ('edge_cost_thr', 'entry_exit_cost', 'miss_rate', 'vis_sim_weight', 'conf_capping_method')
        keys = ('MCF_EDGE_COST_THR', 'MCF_ENTRY_EXIT_COST', 'MCF_MISS_RATE', 'MCF_VIS_SIM_WEIGHT', 'MCF_CONF_CAPPING_METHOD')
        before = {k: self.P[k] for k in keys}
        results, combos, tracks = [], [], []
        lengths = self._length_table_from_dists(self.astar_dists()) if self.dataset.masked else None

        def flush():
            for combo, scores in zip(combos, self._score_series(torch.stack(tracks))):
                results.append(pd.concat([pd.Series(combo, names, dtype=object), scores]))
            combos.clear(); tracks.clear()
        try:
            for ec in ecs:
                for eec in eecs:
                    for mr in mrs:
                        for vsw in vsws:
                            for ccm in ccms:
                                self.P.update(dict(zip(keys, (ec, eec, mr, vsw, ccm))))
                                self.assign_ids(_len_table=lengths)
                                combos.append((ec, eec, mr, vsw, ccm))
                                tracks.append(self._track_dev().clone() if self._solved
                                              else torch.full_like(self.d_x, -1, dtype=torch.int32))
                                if len(tracks) == score_batch:
                                    flush()
            if tracks:
                flush()
        finally:
            self.P.update(before)
        results = pd.concat(results, axis=1).T
        os.makedirs(self.dir, exist_ok=True)
        results.to_csv(f'{self.dir}/MCF_params_results.csv')
        return results

    # ------------------------------------------------------------------ tracking scores on the device
    def _require_scorable(self):
        if not self.labelled:
            raise ValueError("no labels: call set_groundtruth() first")
        if self._shard is not None:
            raise NotImplementedError('tracking scores of a frame-sharded run are not implemented: score in a single '
                                      'process after gather_detections()')
        cap, gcap = int(self.d_x.shape[1]), int(self._gt_dev[0].shape[1])
        if cap > hp.MOT_MAX_SIDE or gcap > hp.MOT_MAX_SIDE:
            raise ValueError(f'{gcap} labels / {cap} detection slots in a frame: the device scorer takes at most '
                             f'{hp.MOT_MAX_SIDE} per frame')
        d = self.nms_min_dist
        if d is None or int(d) != d or not 0 <= d <= hp.MOT_MAX_DIST:
            raise ValueError(f'NON_MAX_SUPRESSION_DIST={d!r}: the device scorer takes an integer in [0, {hp.MOT_MAX_DIST}]')

    def _score_series(self, tracks, events=False):
        """The scores of the associations tracks (i32 [K,F,cap] on the device) as a list of K pd.Series; with events
        (K == 1 at a time is enough for that) also the event log as numpy arrays."""
        from . import mot_metrics
        self._require_scorable()
        F, cap = self.d_x.shape
        if tracks.dim() != 3 or tuple(tracks.shape[1:]) != (F, cap):
            raise ValueError(f'tracks of shape {tuple(tracks.shape)}: expected [K, {F}, {cap}]')
        tracks = tracks.to(device=self.device, dtype=torch.int32).contiguous()
        K = int(tracks.shape[0])
        gx, gy, gc = self._gt_dev
        no, nh = max(self._gt_no, 1), max(int(tracks.max().item()) + 1, 1) if K else 1
        one = hp.mot_scores_scratch_bytes(1, F, cap, gx.shape[1], no, nh, int(self.nms_min_dist))
        if one > 1 << 30:
            raise ValueError(f'scoring one association of {no} label identities x {nh} track identities would take '
                             f'{one / 2 ** 30:.1f} GiB of scratch (limit 1 GiB)')
        chunk = max(1, (1 << 30) // max(one, 1))
        out, log = [], None
        for a in range(0, K, chunk):
            res = hp.mot_scores(tracks[a:a + chunk], self.d_x, self.d_y, self.d_count, self._gt_gid_dev, gx, gy, gc, no, nh,
                                int(self.nms_min_dist), events=events)
            counts, tallies = res[0].cpu().numpy(), res[1].cpu().numpy()
            out += [mot_metrics.scores_from_counts(c, t) for c, t in zip(counts, tallies)]
            if events:
                log = dict(zip(('kind', 'partner', 'fp'), (v.cpu().numpy() for v in res[2:])))
        return (out, log) if events else out

    def get_tracking_metrics(self, events=False):
        """The fifteen MOTChallenge scores (pd.Series, mot_metrics.MOTCHALLENGE_METRICS) of the current association
        against the labels, counted on the device (axt_mot_scores). events=True: also the event log as numpy arrays --
        'kind' u8 [F,gcap] per label slot (0 none, 1 MATCH, 2 SWITCH, 3 MISS), 'partner' i32 [F,gcap] (detection slot,
        -1 none), 'fp' u8 [F,cap] per detection slot."""
        if not self.labelled:
            raise ValueError("no labels: call set_groundtruth() first")
        assert self._solved, "Run .assign_IDs() first!"
        res = self._score_series(self._track_dev()[None], events=events)
        if events:
            return res[0][0], {k: v[0] for k, v in res[1].items()}
        return res[0]

    def score_associations(self, tracks):
        """Scores of K associations of the current detections, i32 tensor [K,F,cap] of track identities (-1 = none):
        DataFrame of K rows, columns mot_metrics.MOTCHALLENGE_METRICS. K is chunked so that the scratch stays under 1 GiB."""
        return pd.DataFrame(self._score_series(tracks))

    def _appearance(self):
        """feature_model's histograms of every detection (device tensors hist f32 [F,cap,180], sums f64 [F,cap]),
        computed once from the centre frames (AxonDetections.py:682-685)."""
        if self._hist is None:
            if hasattr(self.dataset, 'make_resident'):
                self.dataset.make_resident()            # (a host-resident timelapse that has not been streamed yet)
            frames, off = self.dataset.frames, 2
            if not isinstance(self.timepoint_subset, range) and self._shard is None:
                # the centre frames of the subset. (The reference hands the tracker get_frame_and_truedets(i) with i the POSITION in
                # the subset, AxonDetections.py:679-685 -- the image of dataset frame i, not of timepoint_subset[i]; only visible
                # with MCF_VIS_SIM_WEIGHT > 0 under a subset, and not reproduced: the crops here belong to the detections.)
                frames, off = frames[[t + 2 for t in self.timepoint_subset]].contiguous(), 0
            self._hist = hp.box_histograms(frames, self.d_x, self.d_y, self.d_count, t_offset=off,
                                           box=self.axon_box_size)
        return self._hist

    def _mask_dev(self, t=None):
        """The mask as a device grid handle (bit rows + connected components), built once per distinct mask. A static
        mask has one grid; with a time-varying mask `t` selects the grid of the paths that end in detection frame t
        (Timelapse.mask_groups: the reference's mask[t], frame-index quirk included unless
        parameters['REPRODUCE_MASK_FRAME_QUIRK'] is False)."""
        ds = self.dataset
        if ds.mask3d is not None:
            grids, index = self._mask_grids()
            if t is None:
                raise ValueError('the mask changes over time: a frame index is needed')
            return grids[index[t]]
        m = ds.mask2d
        if m is None:
            return None
        if getattr(ds, '_grid', None) is None or ds._grid.conn8 != self.conn8:
            ds._grid = hp.Grid(m, self.conn8, self.device)
        return ds._grid

    def _mask_grids(self):
        """Time-varying mask: (grids, index i32 [frames]) -- one device grid per distinct mask, kept with the timelapse."""
        ds = self.dataset
        quirk = bool(self.P.get('REPRODUCE_MASK_FRAME_QUIRK', True))
        key = (self.conn8, quirk)
        if getattr(ds, '_grids', None) is None or ds._grids[0] != key:
            masks, index = ds.mask_groups(quirk)
            ds._grids = (key, [None if m.all() else hp.Grid(m, self.conn8, self.device) for m in masks], index)
        return ds._grids[1], ds._grids[2]

    def _build_arcs_time_varying(self, dmax, units, vis, src_count):
        """Arcs under a mask that changes over time: the paths of a pair are searched on the mask of its LATER frame
        (AxonDetections.py:557), so one pass of the arc builder per distinct mask -- restricted to the source frames that
        have a target frame under that mask -- and of every pass the arcs whose head frame belongs to it; the union,
        ordered by (tail, gap, head) like a single pass. Global numbering and integer costs do not depend on the pass."""
        grids, index = self._mask_grids()
        F, cap = self.d_x.shape
        gaps = len(dmax)
        dev = self.device
        count = self.d_count
        frame_of = torch.repeat_interleave(torch.arange(F, device=dev), count.long())
        index_d = torch.from_numpy(index).to(dev)
        n_det = int(frame_of.numel())
        parts = []
        for g, grid in enumerate(grids):
            heads = np.nonzero(index == g)[0]
            src = np.zeros(F, bool)
            for gap in range(1, gaps + 1):
                src[heads[heads >= gap] - gap] = True
            sc = torch.where(torch.from_numpy(src).to(dev), count, torch.zeros_like(count))
            if src_count is not None:
                sc = torch.minimum(sc, src_count)
            row_ptr, col, length, gap_a, cost = hp.build_arcs(self.d_x, self.d_y, count, self.dataset.sizey, self.dataset.sizex,
                                                              dmax, units, grid, self.max_px_assoc_dist, self.conn8, vis, None, sc)
            tail = torch.repeat_interleave(torch.arange(n_det, device=dev), (row_ptr[1:n_det + 1] - row_ptr[:n_det]))
            keep = index_d[frame_of[col.long()]] == g
            parts.append((tail[keep], col[keep], length[keep], gap_a[keep], cost[keep]))
        tail, col, length, gap_a, cost = (torch.cat([p[i] for p in parts]) for i in range(5))
        # (tail, gap, head): gap and head get fields as wide as their ranges (a gap > 3 no longer spills into the tail)
        order = torch.argsort((tail * (gaps + 1) + gap_a.long()) * max(n_det, 1) + col.long())
        tail, col, length, gap_a, cost = tail[order], col[order], length[order], gap_a[order], cost[order]
        row_ptr = torch.zeros(F * cap + 1, dtype=torch.int64, device=dev)
        row_ptr[1:n_det + 1] = torch.cumsum(torch.bincount(tail, minlength=n_det), 0)
        row_ptr[n_det + 1:] = row_ptr[n_det]
        return row_ptr, col, length, gap_a, cost

    def _assign_IDs_to_detections(self, len_table=None):
        """AxonDetections.py:631-715 with the tracker replaced by axt_build_arcs + axt_mcf_solve
        (parameters['ASSOCIATION'] = 'mcf', the default and the reference's behaviour) or by the
        frame-to-frame Hungarian variant of BASELINE config 3 ('hungarian'). len_table: path lengths that are already
        known (a path cache, search_MCF_params), read by the flow tracker. True if identities were assigned. The caller has
        dropped the previous association (_drop_association): only what the variant computes is installed."""
        dmax, units = _cost_units_on_device(self.P, self.max_px_assoc_dist, self.device)
        mode = self.P.get('ASSOCIATION', 'mcf')
        if mode == 'hungarian':
            return self._associate_hungarian(dmax, units)
        if mode != 'mcf':
            raise ValueError(f"parameters['ASSOCIATION'] must be 'mcf' or 'hungarian', got {mode!r}")
        return self._associate_mcf(dmax, units, len_table)

    def _appearance_term(self):
        """The appearance term of the link costs as the arc builder takes it; None without one (MCF_VIS_SIM_WEIGHT = 0)."""
        P = self.P
        if not P['MCF_VIS_SIM_WEIGHT']:
            return None
        hist, hsum = self._appearance()
        return dict(hist=hist, hsum=hsum, weight=P['MCF_VIS_SIM_WEIGHT'], miss_rate=P['MCF_MISS_RATE'], thr=P['MCF_EDGE_COST_THR'])

    def _exact_lengths_if_needed(self, dmax, given=None):
        """The path-length table the arc builder reads instead of searching: `given`, the exact lengths, or None."""
        if given is None and self.dataset.masked and max(dmax) - 1 > 250:
            # the hot-path searches of the arc builder cover paths of up to 251 cells (the deployed threshold admits
            # exactly that); wider thresholds take the exact, slower search over the whole range
            return self._length_table_from_dists(self.astar_dists())
        return given

    def _arcs(self, dmax, units, vis, len_table, src_count):
        """(row_ptr, col, length, gap, cost) of hotpath.build_arcs for these detections: one pass, or under a mask that
        changes over time (and without a length table, which already holds every pair's own mask) one pass per mask."""
        varying = self.dataset.mask3d is not None
        if varying and len_table is None:
            return self._build_arcs_time_varying(dmax, units, vis, src_count)
        mask = None if varying else self._mask_dev()
        return hp.build_arcs(self.d_x, self.d_y, self.d_count, self.dataset.sizey, self.dataset.sizex, dmax, units, mask,
                             self.max_px_assoc_dist, self.conn8, vis, len_table, src_count)

    def _associate_hungarian(self, dmax, units):
        """The frame-to-frame variant: installs the tracks and the identity count, both on the device. Returns True."""
        vis = self._appearance_term()
        shard = self._shard                             # set by gather_detections(): solve only this rank's frame pairs
        ctab = None
        if vis is not None or self.dataset.mask3d is not None:
            # the appearance term: the link costs are those of the flow tracker's arcs (axt_build_arcs with d_hist: the same
            # admission, the same integers), scattered into a dense table per frame pair
            # (likewise a mask that changes over time: one pass of the arc builder per distinct mask)
            row_ptr, col, _, gap, cost = self._arcs(dmax, units, vis, self._exact_lengths_if_needed(dmax), None)
            ctab = self._hungarian_cost_table(row_ptr, col, gap, cost, len(dmax))
        mask = self._mask_dev() if (self.dataset.masked and ctab is None) else None
        # (host copies of the tracks are made on first use only, and the count stays on the device)
        self._d_track, self._n_tracks_dev = hp.hungarian_assoc(
            self.d_x, self.d_y, self.d_count, self.dataset.sizey, self.dataset.sizex, dmax, units,
            int(np.rint(self.P['MCF_EDGE_COST_THR'] * 1e6)), self.max_px_assoc_dist, self.conn8,
            *(((shard[0], shard[1]), shard[2]) if shard else (None, None)), mask=mask, ctab=ctab)
        return True

    def _node_costs_int(self, obs, n_det):
        """The integer node costs (axt_arc_cost_int: round(cost * 1e6) << 16 | identity hash): the observation costs on the
        device, beside the arcs' (the numpy version of the same arithmetic took 57 ms for config 4's 319 k detections);
        entry / exit depend on the count and the price only and are kept, read-only: solves and certificates share them."""
        valid = torch.arange(self.d_conf.shape[1], device=self.device)[None, :] < self.d_count[:, None]
        k = torch.arange(n_det, dtype=torch.int64, device=self.device)
        obs_int = _arc_cost_int_torch(torch.round(obs[valid] * 1e6).to(torch.int64), 2, k, 0)
        ee = float(self.P['MCF_ENTRY_EXIT_COST'])
        key = (n_det, ee, str(self.device))
        if _ENTRY_EXIT_CACHE.get('key') != key:
            units = torch.full((n_det,), int(np.rint(ee * 1e6)), dtype=torch.int64, device=self.device)
            entry, exit_ = (_arc_cost_int_torch(units, kind, k, 0).cpu().numpy() for kind in (0, 1))
            entry.setflags(write=False)
            exit_.setflags(write=False)
            _ENTRY_EXIT_CACHE.update(key=key, entry=entry, exit=exit_)
        return obs_int, _ENTRY_EXIT_CACHE['entry'], _ENTRY_EXIT_CACHE['exit']

    def _associate_mcf(self, dmax, units, len_table):
        """The global min-cost flow: installs the tracks (host), the identity count, the total cost and, if asked for, the
        certificate. Returns False, installing nothing, when the flow problem is infeasible."""
        P = self.P
        shard = self._shard                             # set by gather_detections(): build only this rank's arc rows
        obs = hp.obs_costs(self.d_conf, self.d_count, P['MCF_CONF_CAPPING_METHOD'], P['MCF_MAX_CONF_COST'])
        vis = self._appearance_term()
        len_table = self._exact_lengths_if_needed(dmax, len_table)
        src_count = None
        if shard is not None and (self.dataset.masked or vis is not None or len_table is not None):
            # frame-sharded: this rank builds the arc rows of its own frames, one all-gather joins them (the path
            # searches of a masked grid / the appearance distances are the expensive part of the association and shard
            # with the frames). On an all-ones mask the arcs are closed-form and cheaper to rebuild on every rank than to
            # exchange: the all-gather of the detections is then the ONLY collective before the replicated flow solve.
            src_count = torch.zeros_like(self.d_count)
            src_count[shard[0]:shard[1]] = self.d_count[shard[0]:shard[1]]
        row_ptr, col, length, gap, cost = self._arcs(dmax, units, vis, len_table, src_count)
        n_det = int(self._offs[-1])
        if src_count is not None:
            from . import sharded
            row_ptr, col, length, gap, cost = sharded.all_gather_arcs(row_ptr, col, length, gap, cost, n_det, shard[2])
        obs_int, entry_int, exit_int = self._node_costs_int(obs, n_det)
        obs_int, row_ptr_h, col_h, cost_h = hp.to_host(obs_int, row_ptr[:n_det + 1], col, cost)       # (pinned staging: 120 MB at config 4)
        net = (obs_int, entry_int, exit_int, row_ptr_h, col_h, cost_h)
        # parameters['MCF_CERTIFICATE'] (not a key of the reference): also return the node potentials that prove the optimum
        # (axt_mcf_solve_duals) and keep them, with the network they refer to, in self.mcf_certificate
        want_cert = bool(P.get('MCF_CERTIFICATE', False))
        if shard is not None and P.get('MCF_SHARDED_SOLVE', True):
            # frame-sharded: every rank solves its run of time blocks, one all-gather joins the runs (sharded.solve_flow)
            from . import sharded
            res = sharded.solve_flow(*net, P['MCF_MIN_FLOW'], P['MCF_MAX_FLOW'], shard[2], self.device, duals=want_cert)
        else:
            res = hp.mcf_solve(*net, P['MCF_MIN_FLOW'], P['MCF_MAX_FLOW'], duals=want_cert)
        if res is None:
            print('Could not solve the graph for identity association; -> no IDed detections. Try narrowing '
                  'expected identities by updating parameters[`MCF_MIN_FLOW`, `MCF_MAX_FLOW`]. '
                  f"Currently: {P['MCF_MIN_FLOW']} to {P['MCF_MAX_FLOW']}.")
            return False
        if want_cert:
            self.mcf_certificate = dict(obs=net[0].copy(), entry=net[1], exit=net[2], row_ptr=net[3].copy(), col=net[4].copy(),
                                        cost=net[5].copy(), next=res[0], track=res[1], total_cost=res[3], potentials=res[4],
                                        min_flow=P['MCF_MIN_FLOW'], max_flow=P['MCF_MAX_FLOW'])
        _, track, n_tracks, total = res[:4]
        self._track_flat_cache, self.n_ids, self.mcf_total_cost = track, n_tracks, total
        return True

    def _hungarian_cost_table(self, row_ptr, col, gap, cost, gaps):
        """Arcs (CSR by global tail index, global head indices, integer costs) -> i64 [F, cap, gaps, cap] with
        hp.HUNGARIAN_NO_LINK where there is no arc: what axt_hungarian_pairs reads as d_ctab. All on the device."""
        F, cap = self.d_x.shape
        if F * cap * gaps * cap * 8 > 4 << 30:
            raise NotImplementedError(f'the cost table of {F} frames x {cap} detection slots would take '
                                      f'{F * cap * gaps * cap * 8 / 2 ** 30:.1f} GiB')
        dev = self.device
        offs = torch.zeros((F + 1,), dtype=torch.int64, device=dev)
        offs[1:] = torch.cumsum(self.d_count.long(), 0)
        n_det = int(offs[-1].item())
        deg = (row_ptr[1:n_det + 1] - row_ptr[:n_det]).long()
        tail = torch.repeat_interleave(torch.arange(n_det, device=dev), deg, output_size=len(col))
        ft = torch.searchsorted(offs, tail, right=True) - 1
        head = col.long()
        fb = torch.searchsorted(offs, head, right=True) - 1
        tab = torch.full((F, cap, gaps, cap), hp.HUNGARIAN_NO_LINK, dtype=torch.int64, device=dev)
        tab[ft, tail - offs[ft], gap.long() - 1, head - offs[fb]] = cost
        return tab

    @property
    def _offs(self):
        """Start of every frame in the flat (frame-major) detection numbering, i64 [F+1]."""
        return np.concatenate([[0], np.cumsum(self._host_dets()[0])]).astype(np.int64)

    @property
    def _track_flat(self):
        """Trajectory id of every detection in flat numbering on the host, i32 [n_det] (-1: none)."""
        if self._track_flat_cache is None:
            cnt = self._host_dets()[0]
            track_h = self._d_track.cpu().numpy()
            self._track_flat_cache = track_h[np.arange(track_h.shape[1])[None, :] < cnt[:, None]]
        return self._track_flat_cache

    def ided_arrays(self):
        """(frame i32, id i32, conf f32, x i32, y i32) of every IDed detection, frame-major."""
        cnt, conf, x, y = self._host_dets()
        frame_of = np.repeat(np.arange(len(cnt)), cnt)
        k = np.arange(len(frame_of))
        idx_in = k - self._offs[frame_of]
        track = self._track_flat
        sel = track >= 0
        return (frame_of[sel], track[sel], conf[frame_of[sel], idx_in[sel]], x[frame_of[sel], idx_in[sel]],
                y[frame_of[sel], idx_in[sel]])

    def _agg_all_IDed_dets(self):
        """AxonDetections.py:825-842, including (by default) its frame-label quirk: labels are
        column_position//3, so frames after one without IDed detections are labelled one too low.

        The table is dense [n_ids, 3*frames] f64 with NaN where an axon is absent -- its size grows with
        frames x ids, so it is filled on the GPU (axt_ided_table) and copied once into pinned host memory,
        which the DataFrame then wraps without another copy."""
        track = self._track_dev()                                   # i32 [F,cap], -1 = no ID / empty slot
        if self._shard is not None:
            return self._ided_block(track, self._shard[0], self._shard[1])
        key = (int(track.shape[0]), int(track.shape[1]))
        if self._n_ids is None and self._n_tracks_dev is not None and key in _IDS_GUESS:
            # The number of identities is still on the device, and fetching it first would hold the host -- and with it the
            # launches below -- until the GPU has drained the pass. The table is built for the count of the previous pass over
            # a timelapse of this shape (+ a margin) instead, the count travels with it, and rows beyond it are not shown; only
            # if the guess turns out too small is the table built again.
            rows = _IDS_GUESS[key]
            got = _pinned_count()
            got.copy_(self._n_tracks_dev, non_blocking=True)
            vals, wait = hp.ided_table(track, self.d_conf, self.d_x, self.d_y, self.d_count, rows, self.reproduce_label_quirk, None, rows)
            wait()
            n = self._n_ids = int(got[0])
            _IDS_GUESS[key] = (n // 64 + 2) * 64
            if n <= rows:
                return pd.DataFrame(vals[:n], index=_axon_index(np.arange(n)), columns=_ided_columns(len(self)), copy=False)
        n_ids, ids, id_row = self.n_ids, None, None
        if n_ids is not None:
            _IDS_GUESS[key] = (n_ids // 64 + 2) * 64
        if n_ids is None:                                           # adopted from a cache: ids may have gaps
            uniq = torch.unique(track[track >= 0])
            ids = uniq.cpu().numpy()
            n_ids = int(ids[-1]) + 1 if len(ids) else 0
            id_row = torch.full((max(n_ids, 1),), -1, dtype=torch.int32, device=self.device)
            id_row[uniq.long()] = torch.arange(len(ids), dtype=torch.int32, device=self.device)
        vals, wait = hp.ided_table(track, self.d_conf, self.d_x, self.d_y, self.d_count, n_ids, self.reproduce_label_quirk,
                                   id_row, None if ids is None else len(ids))
        df = pd.DataFrame(vals, index=_axon_index(np.arange(n_ids) if ids is None else ids),
                          columns=_ided_columns(len(self)), copy=False)          # built while the copy is in flight
        wait()
        return df

    def _ided_block(self, track, a, b):
        """Frame-sharded runs: the dense table of a timelapse grows with frames x identities, so every rank
        materialises only its own frames [a, b) of it -- the identities alive there (rows) x those frames (columns,
        labelled with their true frame index, no label quirk yet). sharded.assemble_ided_dets_all() joins the blocks
        into exactly the table a single process builds (quirk included); the work and the PCIe traffic per rank stay
        constant as ranks are added."""
        tr = track[a:b]
        alive = torch.unique(tr[tr >= 0])
        id_row = torch.full((max(int(self.n_ids or 0), 1),), -1, dtype=torch.int32, device=self.device)
        id_row[alive.long()] = torch.arange(len(alive), dtype=torch.int32, device=self.device)
        vals, wait = hp.ided_table(tr, self.d_conf[a:b], self.d_x[a:b], self.d_y[a:b], self.d_count[a:b], int(self.n_ids or 0),
                                   False, id_row, len(alive))
        cols = pd.MultiIndex.from_product([range(a, b), ['anchor_x', 'anchor_y', 'conf']], names=('frameID', 'detInfo'))
        self.IDed_dets_block = (a, b)
        df = pd.DataFrame(vals, index=_axon_index(alive.cpu().numpy()), columns=cols, copy=False)
        wait()
        return df

    # ------------------------------------------------------------------ axon reconstructions (AxonDetections.py:924-934)
    def reconstruction_arrays(self, interpolate_missing=True):
        """The axon reconstructions as numpy arrays (the low-level accessor beside ided_arrays()). Per link -- a detection
        and the next detection of its identity within MCF_MAX_NUM_MISSES + 1 frames, in ascending tail order:
        'tail_frame', 'tail_slot', 'head_frame', 'head_slot', 'axon_id', 'gap', 'len' (cells of the link's minimum-cost
        path; max_px_assoc_dist = no path), 'cell_ptr' [n_links+1] and 'cells' (y*W + x along the path, source first: the
        cells astar_dets_paths() holds for that pair). Per interpolated frame (the frames a gap link skips; none with
        interpolate_missing=False): 'interp_axon_id', 'interp_frame', 'interp_x', 'interp_y', 'interp_link' and
        'interp_index' (position along the link's path, _interp_index). The GPU work (hotpath.track_links +
        hotpath.link_paths) runs once per assign_ids() and is cached."""
        if self._shard is not None:
            raise NotImplementedError('axon reconstructions of a frame-sharded run are not implemented: reconstruct in a '
                                      'single process (AxonDetections without gather_detections)')
        if not self._solved:
            raise ValueError('no identities: run assign_ids() first (or the association was infeasible)')
        if self._recon is None:
            self._recon = self._trace_links()
        r = dict(self._recon)
        if not interpolate_missing:
            for k in ('interp_axon_id', 'interp_frame', 'interp_x', 'interp_y', 'interp_link', 'interp_index'):
                r[k] = r[k][:0]
        return r

    def _trace_links(self):
        max_gap = self.P['MCF_MAX_NUM_MISSES'] + 1
        track = self._track_dev()
        F, cap = track.shape
        H, W = self.dataset.sizey, self.dataset.sizex
        links = hp.track_links(track, self.d_count, max_gap)
        if self.dataset.mask3d is not None:
            grids, index = self._mask_grids()           # the mask _masked_dets_paths searches the pair ending in t on
            head_group = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(self.device)
        else:
            grids, head_group = [self._mask_dev()], None
        length, cell_ptr, cells, interp = hp.link_paths(links, self.d_x, self.d_y, H, W, grids, head_group,
                                                        self.max_px_assoc_dist, self.conn8, max_gap)
        links_h, len_h, ptr_h, cells_h, interp_h, track_h = (a.copy() for a in hp.to_host(links, length, cell_ptr, cells,
                                                                                            interp, track))
        tail, head, gap = (links_h[:, k].astype(np.int64) for k in range(3))
        out = dict(tail_frame=tail // cap, tail_slot=tail % cap, head_frame=head // cap, head_slot=head % cap,
                   axon_id=track_h.reshape(-1)[tail].astype(np.int64), gap=gap, len=len_h.astype(np.int64),
                   cell_ptr=ptr_h.astype(np.int64), cells=cells_h.astype(np.int64), max_dist=self.max_px_assoc_dist,
                   shape=(H, W))
        li, kk = np.nonzero(interp_h >= 0) if interp_h.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        c = interp_h[li, kk].astype(np.int64)
        k = kk.astype(np.int64) + 1
        out.update(interp_axon_id=out['axon_id'][li], interp_frame=out['tail_frame'][li] + k, interp_x=c % W,
                   interp_y=c // W, interp_link=li.astype(np.int64), interp_index=_interp_index(k, out['len'][li], gap[li]))
        return out

    def get_axon_reconstructions(self, t=None, axon_name=None, include_history=True, interpolate_missing=True, ymin=0,
                                 ymax=0, xmin=0, xmax=0):
        """The paths the tracked growth cones took (the reference's stub, AxonDetections.py:930-934, in the format its
        caller reads, video_plotting.py:164-168,301-304): a DataFrame with columns (axonID, coord in {'X', 'Y'}, frameID)
        and one row per position along a segment (float, NaN-padded). The segment of frame t of an axon is the
        minimum-cost path from its previous position -- detected, or interpolated with interpolate_missing -- to its
        position at t, both ends included (consecutive segments share a cell); an axon's first frame has none. Without
        interpolate_missing a link across missed frames is one segment, keyed by its head frame; a link without a path
        (farther than max_px_assoc_dist) has none.
        t: None = every frame; include_history: the segments of frames <= t (else == t only). axon_name: a name
        ('Axon_007') or a list of names. Cells outside [ymin, ymax) x [xmin, xmax) are NaN and coordinates are shifted
        by (xmin, ymin), as the caller shifts its anchors; a max of 0 means the frame edge.
        frameID is the detection frame's true position: it does NOT carry the frame-label quirk of IDed_dets_all's
        columns (REPRODUCE_FRAME_LABEL_QUIRK)."""
        r = self.reconstruction_arrays(interpolate_missing)
        seg = _recon_segments(r, interpolate_missing)
        return _recon_frame(seg, r['cells'], r['shape'], t, _name_list(axon_name), include_history, ymin, ymax, xmin, xmax)

    def _reconstruct_axons(self):
        """AxonDetections.py:924-928: the reconstructions of the whole timelapse."""
        return self.get_axon_reconstructions()

    def get_axon_growth(self, interpolate_missing=True):
        """Per axon and frame where it has a detected or interpolated position, indexed by (axonID, frameID): anchor_x,
        anchor_y, conf (NaN where interpolated), interpolated, step_px (moves of the segment ending here -- a diagonal
        move counts 1, as in the tracker's path lengths; 0 at the axon's first frame, NaN where the link has no path),
        length_px (cumulative; NaN from the first unknown step on), and with the timelapse's pixelsize length_um, with
        pixelsize and dt (minutes per frame) speed_um_per_min = step over dt x the frames the step spans. frameID as in
        get_axon_reconstructions (no label quirk)."""
        r = self.reconstruction_arrays(interpolate_missing)
        seg = _recon_segments(r, interpolate_missing)
        frame, ids, conf, x, y = self.ided_arrays()
        return _growth_table(frame, ids, conf, x, y, r, seg, getattr(self.dataset, 'pixelsize', None),
                             getattr(self.dataset, 'dt', None))

    # ------------------------------------------------------------------ target screens (video_plotting.py:170-177,308-309)
    def _require_target(self, ids=False):
        if self._shard is not None:
            raise NotImplementedError('target screens of a frame-sharded run are not implemented: screen in a single '
                                      'process (AxonDetections without gather_detections)')
        if self._target_cells is None:
            raise ValueError('no target: call set_target() first')
        if ids and not self._solved:
            raise ValueError('no identities: run assign_ids() first (or the association was infeasible)')

    def set_target(self, target, reach_px=None):
        """The target of the screen (the reference's StructureScreen.structure_outputchannel_coo, read at
        video_plotting.py:176): (y, x), a bool array [H, W], or an int array [n, 2] of (y, x) cells -- non-empty and inside
        the grid. Sets structure_outputchannel_coo = (y, x): for a region its cell nearest the centroid (ties: the first in
        row-major order). reach_px: a growth cone within this many moves has reached the target (default
        axon_box_size // 2). Drops the cached fields."""
        H, W = self.dataset.sizey, self.dataset.sizex
        cells = _parse_target(target, H, W)
        reach = self.axon_box_size // 2 if reach_px is None else int(reach_px)
        if reach < 0:
            raise ValueError('reach_px must be >= 0')
        self._target_cells, self.reach_px = cells, reach
        self.structure_outputchannel_coo = _region_centre(cells, W)
        self._target_fields, self._target_dets, self._target_path_cache = {}, None, None

    def _target_groups(self):
        """(grids, index): one device grid (None = all ones) per distinct mask, and the group of every frame (None: one)."""
        if self.dataset.mask3d is not None:
            grids, index = self._mask_grids()
            return grids, np.ascontiguousarray(index, np.int32)
        return [self._mask_dev()], None

    def _target_field_of_group(self, g, grid):
        key = (g, self.conn8)
        if key not in self._target_fields:
            H, W = self.dataset.sizey, self.dataset.sizex
            cells = torch.from_numpy(self._target_cells.astype(np.int32)).to(self.device)
            self._target_fields[key] = hp.target_field(cells, H, W, grid, self.conn8)
        return self._target_fields[key]

    def target_field(self, t=None):
        """(off, moves) i32 [H, W] on the device: for every cell the off-mask cells entered and the moves of its
        minimum-cost path to the target (hotpath.target_field), on the mask of detection frame t -- t is needed when the
        mask changes over time (the mask _mask_dev(t) gives). Cached per distinct mask and connectivity."""
        self._require_target()
        grids, index = self._target_groups()
        if index is None:
            return self._target_field_of_group(0, grids[0])
        if t is None:
            raise ValueError('the mask changes over time: a frame index is needed')
        return self._target_field_of_group(int(index[t]), grids[int(index[t])])

    def _target_samples(self):
        """(off, moves) of every detection slot on the device, i32 [F, cap] (-1: empty slot or outside the grid), with the
        fields, grids and per-frame field index they were read from."""
        self._require_target()
        if self._target_dets is None:                               # (valid until the detections or the target change)
            grids, index = self._target_groups()
            fields = [self._target_field_of_group(g, grid) for g, grid in enumerate(grids)]
            if index is None:
                off, moves, d_index = fields[0][0], fields[0][1], None
            else:
                off, moves = torch.stack([f[0] for f in fields]), torch.stack([f[1] for f in fields])
                d_index = torch.from_numpy(index).to(self.device)
            d_off, d_moves = hp.target_sample(off, moves, self.d_x, self.d_y, self.d_count, d_index)
            self._target_dets = (d_off, d_moves, fields, grids, d_index)
        return self._target_dets

    def target_arrays(self):
        """(frame, axon_id, x, y, off, moves) of every IDed detection, frame-major like ided_arrays(): off / moves = the
        target field at the detection (-1 outside the grid)."""
        self._require_target(ids=True)
        d_off, d_moves = self._target_samples()[:2]
        off_h, moves_h = (a.copy() for a in hp.to_host(d_off, d_moves))
        frame, ids, _, x, y = self.ided_arrays()
        cnt = self._host_dets()[0]
        valid = np.arange(off_h.shape[1])[None, :] < cnt[:, None]
        sel = self._track_flat >= 0
        return frame, ids, x, y, off_h[valid][sel], moves_h[valid][sel]

    def get_target_distances(self):
        """Per axon and frame where it has an IDed detection, indexed by (axonID, frameID): anchor_x, anchor_y, conf,
        target_dist_px (moves of the minimum-cost path to the target, a diagonal move counts 1; NaN outside the grid),
        target_off_mask (off-mask cells that path enters), on_mask_route (it enters none), approach_px (the axon's previous
        known distance minus this one; NaN at its first frame), reached (target_dist_px <= reach_px), and with the
        timelapse's pixelsize target_dist_um, with pixelsize and dt (minutes per frame) approach_um_per_min. frameID is
        the true frame (no label quirk), as in get_axon_growth."""
        frame, ids, x, y, off, moves = self.target_arrays()
        conf = self.ided_arrays()[2]
        return _target_table(frame, ids, conf, x, y, off, moves, self.reach_px, getattr(self.dataset, 'pixelsize', None),
                             getattr(self.dataset, 'dt', None))

    def get_target_summary(self):
        """One row per axon: first_frame, last_frame, n_frames, dist_first, dist_last, dist_min, frame_of_min,
        net_approach_px (dist_first - dist_last) and reached_frame (the first frame within reach_px; NaN if never)."""
        frame, ids, _, _, _, moves = self.target_arrays()
        return _target_summary(frame, ids, moves, self.reach_px)

    def _target_paths(self):
        """(cell_ptr i64 [F*cap+1], cells i64) on the host: the target path of every detection slot (CSR)."""
        d_off, d_moves, fields, grids, d_index = self._target_samples()
        if self._target_path_cache is None:
            H, W = self.dataset.sizey, self.dataset.sizex
            ptr, cells = hp.target_paths(fields, grids, self.d_x, self.d_y, d_moves, H, W, d_index, self.conn8)
            self._target_path_cache = tuple(a.astype(np.int64) for a in hp.to_host(ptr, cells))
        return self._target_path_cache

    def _target_path_slots(self, t):
        """(axon ids, slots f*cap+i) of the IDed detections of frame t."""
        cnt = self._host_dets()[0]
        track = self._track_dev()[t].cpu().numpy()[:cnt[t]]
        i = np.nonzero(track >= 0)[0]
        return track[i].astype(np.int64), t * int(self.d_x.shape[1]) + i

    def get_trg_path(self, t, axon_name=None, ymin=0, ymax=0, xmin=0, xmax=0):
        """The paths to the target of the IDed detections of frame t, in the format the reference's consumer indexes its
        canvas with (video_plotting.py:173,308-309): {'Axon_007': (ys, xs)} of int arrays, the detection's cell first, a
        target cell last. axon_name: a name or a list of names. Cells outside [ymin, ymax) x [xmin, xmax) are dropped and
        the others shifted by (ymin, xmin), like get_axon_reconstructions; a max of 0 means the frame edge. A detection
        outside the grid has no path."""
        self._require_target(ids=True)
        if not 0 <= int(t) < len(self):
            raise ValueError(f'frame {t} lies outside the timelapse [0, {len(self)})')
        ptr, cells = self._target_paths()
        ids, slots = self._target_path_slots(int(t))
        H, W = self.dataset.sizey, self.dataset.sizex
        return _trg_path_dict(ids, slots, ptr, cells, (H, W), _name_list(axon_name), ymin, ymax, xmin, xmax)

    # ------------------------------------------------------------------ rendering (video_plotting.py:17-320)
    def render_frames(self, which_dets='IDed', t_y_x_slice=(None, None, None), draw_grid=True, draw_scalebar=False,
                      draw_axon_reconstructions=False, draw_true_dets=False, draw_brightened_bg=False, axon_subset=None,
                      description='', annotate=True, draw_target_paths=False):
        """The annotated frames video_plotting.draw_frame draws, as uint8 RGB on the timelapse's device: torch.uint8
        [T', H', W', 3] for t_y_x_slice = ((tmin, tmax), (ymin, ymax), (xmin, xmax)), None = the whole axis (as draw_all
        takes it). Drawn by one HIP kernel (axt_render_frames), bottom to top: the frame in red, the brightened background
        (draw_brightened_bg), the tile grid (draw_grid), the trails of get_axon_reconstructions(t, include_history=True)
        (draw_axon_reconstructions, 'IDed' only), the paths to the target of get_trg_path(t) in (217, 217, 217) and over them
        the target cells in white, 5 x 5 squares each (draw_target_paths, 'IDed' only, needs set_target()), the ground-truth outlines (draw_true_dets), the dashed boxes of
        get_frame_dets(which_dets, t) in palette[n % 20], their labels 'Ax{n:03}' and the header (annotate), the scale bar
        (draw_scalebar, needs the timelapse's pixelsize). axon_subset: names ('Axon_007') whose boxes, labels and trails
        are drawn. The rules are in DESIGN.md 6.8b; a host-resident timelapse is made resident first."""
        from .render import render_frames
        return render_frames(self, which_dets, t_y_x_slice, draw_grid, draw_scalebar, draw_axon_reconstructions,
                             draw_true_dets, draw_brightened_bg, axon_subset, description, annotate, draw_target_paths)

    def _track_dev(self):
        """Trajectory id of every detection slot on the device, i32 [F,cap] (-1: none)."""
        if self._d_track is None:
            cnt = self._host_dets()[0]
            cap = self.d_conf.shape[1]
            full = np.full((len(cnt), cap), -1, np.int32)
            valid = np.arange(cap)[None, :] < cnt[:, None]
            full[valid] = self._track_flat_cache
            self._d_track = torch.from_numpy(full).to(self.device)
        return self._d_track


def _name_list(axon_name):
    """axon_name of the accessors (None, a name, or a list of names) -> None or a list."""
    return None if axon_name is None else ([axon_name] if isinstance(axon_name, str) else list(axon_name))


_COLUMNS_CACHE = {}
_UNITS_CACHE = {}
_ENTRY_EXIT_CACHE = {}          # the integer entry / exit costs of the last (detection count, price, device)
_IDS_GUESS = {}                 # (frames, capacity) -> rows to build IDed_dets_all for before the count is known
_COUNT_BUF = []


def _pinned_count():
    if not _COUNT_BUF:
        _COUNT_BUF.append(torch.zeros((1,), dtype=torch.int32, pin_memory=True))
    return _COUNT_BUF[0]
_THRS_CACHE = {}


def _conf_thresholds(conf_thr):
    """all_conf_thrs (AxonDetections.py:65-66): the thirteen thresholds of the detection metrics, read-only, per BBOX_THRESHOLD."""
    if conf_thr not in _THRS_CACHE:
        a = np.sort(np.append(np.arange(0.55, 1, .04), conf_thr)).round(2)
        a.setflags(write=False)
        _THRS_CACHE[conf_thr] = a
    return _THRS_CACHE[conf_thr]


def _cost_units_on_device(P, max_px, device):
    """(dmax i32 [gaps], integer cost table i64 [gaps, max_px+1] on `device`) of the transition model for these
    parameters. Cached: the table is a pure function of four parameters, and uploading it from pageable memory in
    the middle of a pass would make the host wait for the detector."""
    key = (P['MCF_VIS_SIM_WEIGHT'], P['MCF_MAX_NUM_MISSES'], P['MCF_MISS_RATE'], P['MCF_EDGE_COST_THR'], max_px, str(device))
    if key not in _UNITS_CACHE:
        table, dmax = transition_cost_table(P, max_px, vis_sim=1.0 if P['MCF_VIS_SIM_WEIGHT'] else 0.0)
        units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
        _UNITS_CACHE[key] = (dmax, torch.from_numpy(units).to(device))
    return _UNITS_CACHE[key]


def _ided_columns(F):
    """MultiIndex (frameID, detInfo) of IDed_dets_all; building it costs more than the rest of the table."""
    if F not in _COLUMNS_CACHE:
        _COLUMNS_CACHE[F] = pd.MultiIndex.from_product([range(F), ['anchor_x', 'anchor_y', 'conf']],
                                                       names=('frameID', 'detInfo'))
    return _COLUMNS_CACHE[F]


_AXON_NAMES = [f'Axon_{i:0>3}' for i in range(2048)]


def _axon_number(name):
    """'Axon_012' -> 12, 'Axon_1234' -> 1234 (names are zero-padded to three digits, not truncated)."""
    return int(str(name).split('_')[-1])


def _axon_index(ids):
    names = [_AXON_NAMES[i] if i < 2048 else f'Axon_{i:0>3}' for i in ids]
    return pd.Index(names, name='axonID')


def _interp_index(k, L, g):
    """Cell index along a link's path of L cells at which the k-th of the g-1 frames a gap-g link skips is placed:
    round(k (L-1) / g), halves up -- the same rule as axt_link_cells."""
    k, L, g = (np.asarray(v, np.int64) for v in (k, L, g))
    return (2 * k * (L - 1) + g) // (2 * g)


def _recon_segments(r, interpolate_missing):
    """reconstruction_arrays() -> the segments, sorted by (axon, frame): dict of arrays axon, frame (where the segment
    ends), start (into r['cells']), n (cells; 0 = the link has no path), step (moves, NaN without a path), span (frames
    the segment covers), interp_end (the segment ends at an interpolated position)."""
    L, g, ptr = r['len'], r['gap'], r['cell_ptr'][:-1]
    has = (L > 0) & (L < r['max_dist'])
    split = has & (g >= 2) if interpolate_missing else np.zeros(len(L), bool)
    whole = ~split
    parts = [dict(axon=r['axon_id'][whole], frame=r['head_frame'][whole], start=ptr[whole], n=np.where(has, L, 0)[whole],
                  step=np.where(has, L - 1, np.nan)[whole], span=g[whole].astype(np.float64),
                  interp_end=np.zeros(int(whole.sum()), bool))]
    for k in range(1, int(g.max()) + 1 if len(g) else 1):
        sel = split & (g >= k)
        Ls, gs = L[sel], g[sel]
        a = _interp_index(k - 1, Ls, gs)
        b = np.where(k == gs, Ls - 1, _interp_index(k, Ls, gs))
        parts.append(dict(axon=r['axon_id'][sel], frame=r['tail_frame'][sel] + k, start=ptr[sel] + a, n=b - a + 1,
                          step=(b - a).astype(np.float64), span=np.ones(len(Ls)), interp_end=k < gs))
    seg = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    order = np.lexsort((seg['frame'], seg['axon']))
    return {key: v[order] for key, v in seg.items()}


def _recon_frame(seg, cells, shape, t, names, include_history, ymin, ymax, xmin, xmax):
    """The DataFrame of get_axon_reconstructions from the segments (host only)."""
    H, W = shape
    keep = seg['n'] > 0
    if t is not None:
        keep &= (seg['frame'] <= t) if include_history else (seg['frame'] == t)
    axon_names = np.array([f'Axon_{int(i):0>3}' for i in seg['axon']], dtype=object)
    if names is not None:
        keep &= np.isin(axon_names, np.asarray(names, dtype=object))
    axon, frame, start, n, axon_names = seg['axon'][keep], seg['frame'][keep], seg['start'][keep], seg['n'][keep], axon_names[keep]
    cols_names = ('axonID', 'coord', 'frameID')
    if len(n) == 0:
        return pd.DataFrame([], columns=pd.MultiIndex.from_arrays([[], [], []], names=cols_names), dtype=np.float64)
    nseg = len(n)
    # columns: per axon (in ascending id) its X columns (ascending frame), then its Y columns
    first = np.r_[True, axon[1:] != axon[:-1]]
    grp = np.cumsum(first) - 1
    g_start = np.nonzero(first)[0]
    g_count = np.diff(np.r_[g_start, nseg])
    xcol = 2 * g_start[grp] + (np.arange(nseg) - g_start[grp])
    ycol = xcol + g_count[grp]
    offs = np.r_[0, np.cumsum(n)]
    segi = np.repeat(np.arange(nseg), n)
    rows = np.arange(offs[-1]) - offs[segi]
    c = cells[start[segi] + rows]
    X, Y = (c % W).astype(np.float64), (c // W).astype(np.float64)
    ymax, xmax = (ymax or H), (xmax or W)
    out = (Y < ymin) | (Y >= ymax) | (X < xmin) | (X >= xmax)
    X[out], Y[out] = np.nan, np.nan
    arr = np.full((int(n.max()), 2 * nseg), np.nan)
    arr[rows, xcol[segi]] = X - xmin
    arr[rows, ycol[segi]] = Y - ymin
    col_axon = np.empty(2 * nseg, dtype=object)
    col_coord = np.empty(2 * nseg, dtype=object)
    col_frame = np.empty(2 * nseg, np.int64)
    col_axon[xcol], col_axon[ycol] = axon_names, axon_names
    col_coord[xcol], col_coord[ycol] = 'X', 'Y'
    col_frame[xcol], col_frame[ycol] = frame, frame
    columns = pd.MultiIndex.from_arrays([col_axon, col_coord, col_frame], names=cols_names)
    return pd.DataFrame(arr, columns=columns, copy=False)


def _growth_table(frame, ids, conf, x, y, r, seg, pixelsize, dt):
    """The DataFrame of get_axon_growth from the IDed detections and the segments (host only)."""
    ni = len(r['interp_frame'])
    a = np.concatenate([np.asarray(ids, np.int64), r['interp_axon_id']])
    f = np.concatenate([np.asarray(frame, np.int64), r['interp_frame']])
    ax = np.concatenate([np.asarray(x, np.float64), r['interp_x'].astype(np.float64)])
    ay = np.concatenate([np.asarray(y, np.float64), r['interp_y'].astype(np.float64)])
    cf = np.concatenate([np.asarray(conf, np.float64), np.full(ni, np.nan)])
    interp = np.r_[np.zeros(len(frame), bool), np.ones(ni, bool)]
    order = np.lexsort((f, a))
    a, f, ax, ay, cf, interp = a[order], f[order], ax[order], ay[order], cf[order], interp[order]
    n = len(a)
    first = np.r_[True, a[1:] != a[:-1]] if n else np.zeros(0, bool)
    # step / span of the segment that ends at (axon, frame)
    step, span = np.full(n, np.nan), np.full(n, np.nan)
    if n and len(seg['axon']):
        key_rows = a * (int(f.max()) + 2) + f
        key_seg = seg['axon'] * (int(f.max()) + 2) + seg['frame']
        pos = np.searchsorted(key_rows, key_seg)                     # (rows are sorted by (axon, frame): keys ascend)
        ok = (pos < n) & (key_rows[np.minimum(pos, n - 1)] == key_seg)
        step[pos[ok]], span[pos[ok]] = seg['step'][ok], seg['span'][ok]
    step[first] = 0.0
    # cumulative per axon; NaN from the first unknown step on
    grp = np.cumsum(first) - 1
    cs = np.cumsum(np.nan_to_num(step))
    base = (cs - np.nan_to_num(step))[first][grp] if n else cs
    unknown = np.cumsum(np.isnan(step))
    unknown_before = (unknown - np.isnan(step))[first][grp] if n else unknown
    length = np.where(unknown - unknown_before > 0, np.nan, cs - base)
    data = {'anchor_x': ax, 'anchor_y': ay, 'conf': cf, 'interpolated': interp, 'step_px': step, 'length_px': length}
    if pixelsize is not None:
        data['length_um'] = length * float(pixelsize)
        if dt is not None:
            data['speed_um_per_min'] = step * float(pixelsize) / (float(dt) * span)
    index = pd.MultiIndex.from_arrays([np.array([f'Axon_{int(i):0>3}' for i in a], dtype=object), f],
                                      names=('axonID', 'frameID'))
    return pd.DataFrame(data, index=index)


def _parse_target(target, H, W):
    """set_target's argument -> the sorted unique cells y*W + x (i64), validated."""
    a = np.asarray(target)
    if a.dtype == bool:
        if a.shape != (H, W):
            raise ValueError(f'a target mask must have the grid\'s shape {(H, W)}, got {a.shape}')
        yx = np.argwhere(a)
    elif a.ndim == 1 and a.size == 2:
        yx = a.reshape(1, 2)
    elif a.ndim == 2 and a.shape[1] == 2:
        yx = a
    else:
        raise ValueError('target must be (y, x), a bool array [H, W] or an int array [n, 2] of (y, x)')
    if not (np.issubdtype(yx.dtype, np.integer) or (yx.size and np.all(yx == np.floor(yx)))) and yx.size:
        raise ValueError('target cells must be integers')
    yx = yx.astype(np.int64)
    if len(yx) == 0:
        raise ValueError('the target is empty')
    if (yx[:, 0] < 0).any() or (yx[:, 0] >= H).any() or (yx[:, 1] < 0).any() or (yx[:, 1] >= W).any():
        raise ValueError(f'target cells must lie inside the grid [0, {H}) x [0, {W})')
    return np.unique(yx[:, 0] * W + yx[:, 1])


def _region_centre(cells, W):
    """(y, x) of the cell nearest the centroid of the cells (sorted y*W + x); ties: the first in row-major order."""
    y, x = cells // W, cells % W
    n = len(cells)
    d2 = (n * y - y.sum()) ** 2 + (n * x - x.sum()) ** 2          # n^2 x the squared distance, in integers
    k = int(np.argmin(d2))
    return int(y[k]), int(x[k])


def _axon_names(a):
    return np.array([f'Axon_{int(i):0>3}' for i in a], dtype=object)


def _target_table(frame, ids, conf, x, y, off, moves, reach_px, pixelsize, dt):
    """The DataFrame of get_target_distances from the IDed detections and their field samples (host only)."""
    a, f = np.asarray(ids, np.int64), np.asarray(frame, np.int64)
    order = np.lexsort((f, a))
    a, f = a[order], f[order]
    ax, ay, cf = (np.asarray(v, np.float64)[order] for v in (x, y, conf))
    off, moves = np.asarray(off, np.int64)[order], np.asarray(moves, np.int64)[order]
    n = len(a)
    known = moves >= 0
    dist = np.where(known, moves, np.nan).astype(np.float64)
    offc = np.where(known, off, np.nan).astype(np.float64)
    first = np.r_[True, a[1:] != a[:-1]] if n else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(n), 0)) if n else np.zeros(0, np.int64)
    # the last earlier row of the same axon with a known distance
    last_known = np.maximum.accumulate(np.where(known, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    prev = np.r_[-1, last_known[:-1]] if n else last_known
    has_prev = prev >= start
    pk = np.maximum(prev, 0)
    approach = np.where(has_prev & known, dist[pk] - dist, np.nan) if n else dist
    span = np.where(has_prev, f - f[pk], 1).astype(np.float64) if n else dist
    data = {'anchor_x': ax, 'anchor_y': ay, 'conf': cf, 'target_dist_px': dist, 'target_off_mask': offc,
            'on_mask_route': known & (off == 0), 'approach_px': approach, 'reached': known & (moves <= int(reach_px))}
    if pixelsize is not None:
        data['target_dist_um'] = dist * float(pixelsize)
        if dt is not None:
            data['approach_um_per_min'] = approach * float(pixelsize) / (float(dt) * span)
    index = pd.MultiIndex.from_arrays([_axon_names(a), f], names=('axonID', 'frameID'))
    return pd.DataFrame(data, index=index)


def _target_summary(frame, ids, moves, reach_px):
    """The DataFrame of get_target_summary (host only): one row per axon, in ascending id."""
    a, f = np.asarray(ids, np.int64), np.asarray(frame, np.int64)
    order = np.lexsort((f, a))
    a, f, moves = a[order], f[order], np.asarray(moves, np.int64)[order]
    dist = np.where(moves >= 0, moves, np.nan).astype(np.float64)
    uniq, start, count = np.unique(a, return_index=True, return_counts=True)
    cols = {k: [] for k in ('first_frame', 'last_frame', 'n_frames', 'dist_first', 'dist_last', 'dist_min', 'frame_of_min',
                            'net_approach_px', 'reached_frame')}
    for s0, c in zip(start, count):
        d, fr = dist[s0:s0 + c], f[s0:s0 + c]
        ok = ~np.isnan(d)
        k = int(np.argmin(np.where(ok, d, np.inf))) if ok.any() else -1
        hit = np.nonzero(ok & (d <= int(reach_px)))[0]
        cols['first_frame'].append(int(fr[0])); cols['last_frame'].append(int(fr[-1])); cols['n_frames'].append(int(c))
        cols['dist_first'].append(d[0]); cols['dist_last'].append(d[-1])
        cols['dist_min'].append(d[k] if k >= 0 else np.nan)
        cols['frame_of_min'].append(float(fr[k]) if k >= 0 else np.nan)
        cols['net_approach_px'].append(d[0] - d[-1])
        cols['reached_frame'].append(float(fr[hit[0]]) if len(hit) else np.nan)
    return pd.DataFrame(cols, index=pd.Index(_axon_names(uniq), name='axonID'))


def _trg_path_dict(ids, slots, cell_ptr, cells, shape, names, ymin, ymax, xmin, xmax):
    """get_trg_path's dict from the CSR target paths (host only): axon ids and slots of one frame's IDed detections."""
    H, W = shape
    ymax, xmax = (ymax or H), (xmax or W)
    out = {}
    for k, s0 in zip(ids, slots):
        name = f'Axon_{int(k):0>3}'
        if names is not None and name not in names:
            continue
        c = cells[cell_ptr[s0]:cell_ptr[s0 + 1]]
        if len(c) == 0:
            continue
        ys, xs = c // W, c % W
        keep = (ys >= ymin) & (ys < ymax) & (xs >= xmin) & (xs < xmax)
        out[name] = ((ys[keep] - ymin).astype(np.int64), (xs[keep] - xmin).astype(np.int64))
    return out


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _lsr(x, s):
    """logical right shift of an int64 tensor holding uint64 bits"""
    return (x >> s) & ((1 << (64 - s)) - 1)


def _arc_cost_int_torch(units, kind, a, b):
    """axt_arc_cost_int on int64 device tensors (units = round(cost*1e6) already)."""
    def s64(v):                                   # python int -> signed 64-bit two's complement
        v &= 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v
    x = (a << 30) ^ b ^ s64(kind << 60)
    x = x + s64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * s64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * s64(0x94D049BB133111EB)
    x = x ^ _lsr(x, 31)
    return units * 65536 + (x & 0xFFFF)


def _arc_cost_int_vec(cost, kind, a, b):
    """Vectorised axt_arc_cost_int (include/axtrack_hip.h)."""
    with np.errstate(over='ignore'):
        key = (np.uint64(kind) << np.uint64(60)) ^ (np.asarray(a, np.uint64) << np.uint64(30)) ^ np.asarray(b, np.uint64)
        pert = (_splitmix64(key) & np.uint64(0xFFFF)).astype(np.int64)
    return np.rint(np.asarray(cost, np.float64) * 1e6).astype(np.int64) * 65536 + pert
