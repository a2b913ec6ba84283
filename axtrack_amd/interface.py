"""Public API of the reference (axtrack/interface.py:38-215) on the MI355X hot path:

    parameters, model, stnd_scaler = setup_inference(dest_dir)
    timelapse = prepare_input_data(imseq_fname, parameters, dest_dir, inference_data_dir, stnd_scaler, ...)
    axon_dets = inference(timelapse, model, dest_dir, parameters, ...)
    axon_dets.IDed_dets_all

Same names, argument meaning and return values as the reference, so examples/test.py runs
against this package by changing its import. Differences are confined to where the reference
depends on assets that are not redistributable (the weights file): `setup_inference` takes the weights explicitly.
`prepare_input_data` also accepts arrays, and reads .tif files with the package's own reader (tiff.py), not tifffile.
"""
import glob
import os
import pickle
import warnings

import numpy as np
import torch

from . import params as _params
from .detections import AxonDetections
from .hotpath import Detector
from . import hotpath as _hp
from . import tiff as _tiff
from .timelapse import (Timelapse, preprocess, pad_mask, estimate_stnd_scaler, frame_scales, load_labels_csv,
                        contiguous_runs)

# config.py:5,8 -- the directory that holds examples/ and deployed_model/ (the reference's package root)
PKG_DIR = os.path.abspath(os.path.join(os.path.dirname(__file__), '..')) + '/'
DEPLOYED_MODEL_DIR = PKG_DIR + 'deployed_model/'


def _load_state_dict(weights):
    if isinstance(weights, dict):
        return weights.get('state_dict', weights)
    if os.path.isdir(weights):
        files = sorted(glob.glob(f'{weights}/*.pth'))
        weights = files[0]                       # IndexError if none, like utils.py:270
    ckpt = torch.load(weights, map_location='cpu')
    return ckpt['state_dict']                    # utils.py:260,272


def setup_inference(dest_dir, print_params=False, num_workers=3, device='cuda:0', weights=None, max_batch=256):
    """interface.py:38-77. `weights`: a state_dict, a checkpoint file or a directory holding one. Default, in this order:
    $AXTRACK_MODEL_DIR, then {PKG_DIR}/deployed_model/ as in the reference (interface.py:29, utils.py:269-272: the first
    *.pth of the directory) -- the reference's E1000.pth is an external download, so that directory is empty until the
    user puts the checkpoint there. The standardization scaler is deployed_model/train_stnd_scaler.pkl when that file is
    there (interface.py:66-67), else its known content ('zscore', (0.015176106, 0.009456525))."""
    parameters = _params.load_parameters()
    parameters['NUM_WORKERS'] = num_workers
    parameters['DEVICE'] = device
    torch.manual_seed(parameters['SEED'])
    model_dir = None
    if weights is None:
        for cand in (os.environ.get('AXTRACK_MODEL_DIR'), DEPLOYED_MODEL_DIR):
            if cand and (os.path.isfile(cand) or glob.glob(f'{cand}/*.pth')):
                weights = model_dir = cand
                break
        else:
            raise FileNotFoundError(f'no detector weights: pass weights=<state_dict | .pth | dir>, set AXTRACK_MODEL_DIR, or put the '
                                    f'checkpoint (*.pth) into {DEPLOYED_MODEL_DIR} as the reference\'s README does')
    model = Detector(_load_state_dict(weights), max_batch=max_batch, device=device)
    if print_params:
        for k, v in parameters.items():
            print(f'{k:28} {v}')
    os.makedirs(dest_dir, exist_ok=True)
    stnd_scaler = _params.DEPLOYED_STND_SCALER
    for d in (model_dir if model_dir and os.path.isdir(model_dir) else None, DEPLOYED_MODEL_DIR):
        if d and os.path.exists(f'{d}/train_stnd_scaler.pkl'):
            with open(f'{d}/train_stnd_scaler.pkl', 'rb') as f:
                stnd_scaler = pickle.load(f)
            break
    return parameters, model, stnd_scaler


def prepare_input_data(imseq_fname, parameters, dest_dir, inference_data_dir, stnd_scaler, mask_fname=None,
                       use_cached_datasets='to', check_preproc=False, input_metadata={}):
    """interface.py:79-168. imseq_fname: a .tif/.npy file name inside inference_data_dir or a raw
    uint16 array [T,H,W]; mask_fname: .npy file name, bool array [H,W] or [T,H,W], or None.
    input_metadata['pad'] = p adds p zero pixels on all four sides (interface.py:126-128, Timelapse.py:224-234).
    use_cached_datasets: 'to' writes '{dest_dir}/{name}_dataset_cached.pkl', 'from' reads it (this package's file or
    one the reference wrote) instead of preprocessing, None does neither (Timelapse.py:435-449).
    check_preproc=True (interface.py:159-167): the reference samples every preprocessing step of the first and the last
    time point into '{dest_dir}/{name}_preproc_data.csv' (utils.save_preproc_metrics) and plots them against the training
    data's (train_preproc_data.csv, an external asset). The statistics file is written here in the same layout; the
    comparison plot is out of scope (plotting), which a warning says."""
    name = input_metadata.get('name', 'timelapse')
    if use_cached_datasets not in ('to', 'from', None):
        raise ValueError(f"use_cached_datasets must be 'to', 'from' or None, got {use_cached_datasets!r}")
    if use_cached_datasets == 'from':
        return Timelapse.from_cache(dest_dir, name, device=parameters['DEVICE'])
    if isinstance(imseq_fname, str):
        path = os.path.join(inference_data_dir, imseq_fname)
        if path.endswith('.npy'):
            imseq = np.load(path)
        else:
            # the native reader (tiff.py): the stack stays on the device, int16-viewed raw counts, as preprocess takes it
            imseq = _tiff.read_stack(path, device=parameters['DEVICE'], to_host=False)
    else:
        imseq = np.asarray(imseq_fname)
    mask = None
    if isinstance(mask_fname, str) and not mask_fname.endswith('None'):
        mask = np.load(os.path.join(inference_data_dir, mask_fname))
    elif mask_fname is not None and not isinstance(mask_fname, str):
        mask = np.asarray(mask_fname)
    pad = input_metadata.get('pad')
    pad = [pad] * 4 if pad else None                                     # interface.py:126-128
    frames = preprocess(imseq, mask, offset=input_metadata.get('intensity_offset'),
                        clip=input_metadata.get('clip_intensity'), log_correct=parameters.get('LOG_CORRECT', True),
                        scale=stnd_scaler[1][0], device=parameters['DEVICE'], pad=pad)
    mask_raw = mask
    if pad:
        mask = pad_mask(mask, pad, imseq.shape)
    timelapse = Timelapse(frames, name=name, mask=mask, temporal_context=parameters['TEMPORAL_CONTEXT'],
                          tilesize=parameters['TILESIZE'], device=parameters['DEVICE'],
                          pixelsize=input_metadata.get('pixelsize'), dt=input_metadata.get('dt_min'),
                          incubation_time=input_metadata.get('incubation_time_min'))
    if use_cached_datasets == 'to':
        timelapse.to_cache(dest_dir)
    if check_preproc:
        if isinstance(imseq, torch.Tensor):                              # (the statistics are sampled on the host)
            imseq = imseq.cpu().numpy().view(np.uint16)
        fname = save_preproc_metrics(dest_dir, name, imseq, mask_raw, input_metadata, parameters, stnd_scaler)     # (before padding, as the 'Original' step of the reference is taken after it: zero margins only add zeros)
        warnings.warn(f'check_preproc: the preprocessing statistics are in {fname}; the comparison plot against the training '
                      f'data (ml_plotting.plot_preprocessed_input_data, train_preproc_data.csv) is out of scope of axtrack_amd')
    return timelapse


def _read_stack(source, what, device='cuda:0'):
    """A .npy file, a .tif / .tiff file through the native reader (tiff.py; tifffile only for what that refuses, where
    it is importable), or the array itself. `what` names the file's role in an error."""
    if not isinstance(source, str):
        return np.asarray(source)
    if source.endswith('.npy'):
        return np.load(source)
    try:
        return _tiff.read_stack(source, device=device)
    except _tiff.TiffUnsupported as e:
        raise _tiff.TiffUnsupported(f'{what} {source}: {e}') from e


def process_timelapse(src, dest_basename, timeslice=None, offset=0, mask=None, second_mask=None, to_shape=None, H_slice=None,
                      W_slice=None, device='cuda:0', **write_options):
    """data_prep_nbs/01_process_training_timelapses.ipynb's process_timelapses for one recording, on the device: the step
    between segment_mask and prepare_training_data, which "may also be used to preprocess inference data".
    -> (stack as int16-viewed uint16 [T,H,W] on the device, mask as a bool numpy array or None).

    src: a .tif name (read_tiff), a .npy name or an array; timeslice: (start, stop) frames. offset: subtracted,
    saturating -- values below it become 0. second_mask, then mask (.npy names or arrays, True = keep): pixels outside
    become 0. to_shape (H, W): zero padding of (to - size) // 2 on BOTH sides of an axis, exactly as the notebook pads,
    so an odd difference ends one short of to_shape; a to_shape smaller than the frames raises. H_slice / W_slice: (start,
    stop) behind the padding; the mask is padded and sliced alike. {dest_basename}.tif is written by write_tiff
    (write_options: rows_per_strip, predictor, bigtiff, deflate, description, level; the notebook's bigtiff=True is not
    forced), the adjusted mask by np.save as {dest_basename}.npy."""
    _hp._require_gpu()
    dev = torch.device(device)
    if _tiff.is_tiff_name(src):
        T = _tiff.tiff_info(src).shape[0]
        frames = None if timeslice is None else range(*slice(*timeslice).indices(T))
        stack = _tiff.read_tiff(src, frames=frames, device=dev)
    else:
        a = np.load(src) if isinstance(src, str) else src
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a)
            if a.dtype not in (np.uint16, np.int16):
                raise TypeError(f'the timelapse is {a.dtype}, not uint16')
            a = torch.from_numpy(np.ascontiguousarray(a).view(np.int16))
        stack = a.to(dev)
        if timeslice is not None:
            stack = stack[timeslice[0]:timeslice[1]]
    if stack.dim() != 3:
        raise ValueError(f'the timelapse must be [T,H,W], got {tuple(stack.shape)}')
    s = stack.to(torch.int32) & 0xffff                                    # the raw counts as numbers
    s = (s - int(offset)).clamp_(min=0)

    def load_mask(m):
        m = np.load(m) if isinstance(m, str) else np.asarray(m)
        if m.shape != tuple(s.shape[1:]):
            raise ValueError(f'a mask of shape {m.shape} on frames of {tuple(s.shape[1:])}')
        return m.astype(bool)
    if second_mask is not None:
        s[:, ~torch.from_numpy(load_mask(second_mask)).to(dev)] = 0
    if mask is not None:
        mask = load_mask(mask)
        s[:, ~torch.from_numpy(mask).to(dev)] = 0
    if to_shape is not None:
        ph, pw = (int(to_shape[0]) - s.shape[1]) // 2, (int(to_shape[1]) - s.shape[2]) // 2
        if ph < 0 or pw < 0:
            raise ValueError(f'to_shape {tuple(to_shape)} is smaller than the frames of {tuple(s.shape[1:])}: padding only')
        s = torch.nn.functional.pad(s, (pw, pw, ph, ph))
        if mask is not None:
            mask = np.pad(mask, ((ph, ph), (pw, pw)), mode='constant')
    for axis, sl in ((1, H_slice), (2, W_slice)):
        if sl is not None:
            s = s.narrow(axis, *_slice_start_length(sl, s.shape[axis]))
            if mask is not None:
                mask = mask[sl[0]:sl[1]] if axis == 1 else mask[:, sl[0]:sl[1]]
    out = torch.where(s >= 32768, s - 65536, s).to(torch.int16).contiguous()     # (0..65535 as int16-viewed uint16)
    _tiff.write_tiff(f'{dest_basename}.tif', out, **write_options)
    if mask is not None:
        np.save(f'{dest_basename}.npy', mask)
    return out, mask


def _slice_start_length(sl, size):
    start, stop, _ = slice(sl[0], sl[1]).indices(size)
    return start, max(stop - start, 0)


def prepare_training_data(parameters, skip_test=False, **overrides):
    """core_functionality.setup_data (:15-59): the labelled train and test timelapses of one recording -> (train, test), test
    None with skip_test. Keys read from `parameters` (each can be overridden by keyword): TIMELAPSE_FILE (.npy, a uint16
    array [T,H,W], or .tif through the native reader), LABELS_FILE (the reference's axon_anchor_labels.csv), MASK_FILE (.npy, .tif of 0 / non-0 samples, an
    array, None or a name ending in 'None'), TRAIN_TIMEPOINTS, TEST_TIMEPOINTS (input frame numbers), OFFSET, CLIP_LOWERLIM,
    PAD (top, right, bottom, left), LOG_CORRECT, STANDARDIZE, STANDARDIZE_FRAMEWISE, TEMPORAL_CONTEXT, TILESIZE, CACHE, DEVICE.

    With STANDARDIZE[1] None the train scaler is estimated from ALL frames of the file (estimate_stnd_scaler, as
    Timelapse._standardize runs before the time points are sliced), else the passed scaler is used; the test set gets
    train.stnd_scaler (:58). Frame-wise, that is (name, None) and every frame is divided by its own std / max. Each set is
    the block of input frames [min(tp) - context, max(tp) + context] with its labels at the time points; this package's
    Timelapse is one dense contiguous stack, so a time-point list with a gap raises ValueError naming the runs (call once
    per run). CACHE: a directory that receives train_stnd_scaler.pkl (Timelapse.py:320-323), the file setup_inference
    looks for next to the weights."""
    P = dict(parameters)
    P.update(overrides)
    device, context = P.get('DEVICE', 'cuda:0'), int(P.get('TEMPORAL_CONTEXT', 2))
    imseq = _read_stack(P['TIMELAPSE_FILE'], 'the timelapse', device)
    if imseq.ndim != 3:
        raise ValueError(f'the timelapse must be [T,H,W], got {imseq.shape}')
    T = imseq.shape[0]
    mask = P.get('MASK_FILE')
    mask = None if mask is None or (isinstance(mask, str) and mask.endswith('None')) else _read_stack(mask, 'the mask', device)
    if mask is not None and np.ndim(mask) == 3 and len(mask) == 1 and T != 1:
        mask = mask[0]                                                    # (a mask file of one page is the static mask)
    pad = P.get('PAD')
    pad = [int(v) for v in pad] if pad is not None and any(pad) else None
    H = imseq.shape[1] + (pad[0] + pad[2] if pad else 0)
    W = imseq.shape[2] + (pad[1] + pad[3] if pad else 0)
    labels = load_labels_csv(P['LABELS_FILE'], pad=pad, shape=(H, W))
    name, passed = P.get('STANDARDIZE', ('zscore', None))
    framewise = bool(P.get('STANDARDIZE_FRAMEWISE', False))
    if not name:
        raise ValueError('STANDARDIZE[0] must be \'zscore\' or \'0to1\': the detector reads standardised frames')
    if framewise and passed is not None:
        raise ValueError('a passed scaler applies to timelapse-wide standardisation only: with STANDARDIZE_FRAMEWISE pass '
                         '(name, None)')
    pre = dict(offset=P.get('OFFSET'), clip=P.get('CLIP_LOWERLIM'), log_correct=P.get('LOG_CORRECT', True), device=device)
    per_frame = None
    if passed is None:
        stnd_scaler, per_frame = estimate_stnd_scaler(imseq, mask, standardize=name, framewise=framewise, **pre)
    else:
        stnd_scaler = (name, (float(passed[0]), float(passed[1])))
    scales = frame_scales(stnd_scaler, per_frame)

    def one_set(which, timepoints):
        runs = contiguous_runs(timepoints)
        if not runs:
            raise ValueError(f'{which}_TIMEPOINTS is empty')
        if len(runs) > 1:
            raise ValueError(f'{which}_TIMEPOINTS has gaps: a Timelapse is one contiguous block of frames. Call once per run: '
                             f'{[f"{a}..{b}" for a, b in runs]}')
        a, b = runs[0][0] - context, runs[0][1] + context + 1
        if a < 0 or b > T:
            raise ValueError(f'{which}_TIMEPOINTS {runs[0][0]}..{runs[0][1]} need the input frames {a}..{b - 1}; the file has 0..{T - 1}')
        if b - context > len(labels):
            raise ValueError(f'{P["LABELS_FILE"]} has {len(labels)} rows; {which}_TIMEPOINTS reach frame {b - context - 1}')
        m = mask[a:b] if mask is not None and np.ndim(mask) == 3 else mask
        frames = preprocess(imseq[a:b], m, scale=scales if np.ndim(scales) == 0 else scales[a:b], pad=pad, **pre)
        if pad:
            m = pad_mask(m, pad, imseq[a:b].shape)
        return Timelapse(frames, name=which.lower(), mask=m, temporal_context=context, tilesize=P.get('TILESIZE', 512),
                         device=device, labels=labels[a + context:b - context], stnd_scaler=stnd_scaler)

    train = one_set('TRAIN', P['TRAIN_TIMEPOINTS'])
    if P.get('CACHE'):
        os.makedirs(P['CACHE'], exist_ok=True)
        with open(f"{P['CACHE']}/train_stnd_scaler.pkl", 'wb') as f:
            pickle.dump(train.stnd_scaler, f)
    test = None if skip_test else one_set('TEST', P['TEST_TIMEPOINTS'])
    return train, test


def save_preproc_metrics(dest_dir, name, imseq, mask, input_metadata, parameters, stnd_scaler, n_samples=int(1e6)):
    """utils.save_preproc_metrics (utils.py:90-110) for the steps Timelapse keeps when it plots (Timelapse.py:238-241,250-253,
    260-263,316-319): 'Original' (scaled to [0,1], masked, offset), 'Clipped', 'Log-Adjusted', 'Standardized (frame-wize: ..)',
    each sampled at n_samples random pixels of the first and of the last time point (timepoints[0] / timepoints[-1]: input
    frames temporal_context and T - 1 - temporal_context). Columns (name, step, 't_0' | 't_-1') as in the reference.
    Every step is the fused preprocessing kernel with the later steps switched off (axt_preprocess_u16)."""
    import pandas as pd
    tc = int(parameters['TEMPORAL_CONTEXT'])
    a = np.asarray(imseq)
    two = np.ascontiguousarray(a[[tc, a.shape[0] - 1 - tc]])
    m = None if mask is None else (np.asarray(mask)[[tc, a.shape[0] - 1 - tc]] if np.asarray(mask).ndim == 3 else mask)
    off, clip = input_metadata.get('intensity_offset'), input_metadata.get('clip_intensity')
    log_correct, scale = parameters.get('LOG_CORRECT', True), stnd_scaler[1][0]
    steps = [('Original', dict(clip=0, log_correct=False, scale=1.0)), ('Clipped', dict(clip=clip, log_correct=False, scale=1.0))]
    if log_correct:
        steps.append(('Log-Adjusted', dict(clip=clip, log_correct=True, scale=1.0)))
    if stnd_scaler[0]:
        steps.append((f"Standardized (frame-wize: {parameters.get('STANDARDIZE_FRAMEWISE', False)})",
                      dict(clip=clip, log_correct=log_correct, scale=scale)))
    idx = np.random.default_rng().choice(two[0].size, int(n_samples))
    samples = []
    for step, kw in steps:
        out = preprocess(two, m, offset=off, device=parameters['DEVICE'], **kw).cpu().numpy()
        samples.append(pd.Series(out[0].ravel()[idx], name=(name, step, 't_0')))
        samples.append(pd.Series(out[1].ravel()[idx], name=(name, step, 't_-1')))
    fname = f'{dest_dir}/{name}_preproc_data.csv'
    pd.concat(samples, axis=1).to_csv(fname)
    return fname


def visualize_inference(axon_dets, which_dets='IDed', **kwargs):
    """interface.py:217-320 renders every frame with matplotlib and encodes a video (video_plotting.draw_all): plotting is
    out of scope of this package ("Out of scope"). Everything it would draw is on the object it is given."""
    raise NotImplementedError(
        'visualize_inference (frame rendering / video encoding, axtrack/video_plotting.py) is out of scope of axtrack_amd. '
        'What it draws is available: axon_dets.IDed_dets_all, axon_dets.get_frame_dets(which, t), axon_dets.dataset.mask; '
        "the caches written by inference(..., *_cache='to') are in the reference's layouts, so the reference's own "
        'visualize_inference can read them. axtrack_amd.render_inference draws the annotated frames on the GPU and '
        'writes PNG frames, one animated PNG, or with video=True an MJPEG AVI.')


def inference(timelapse, model, dest_dir, parameters, detections_cache='to', astar_paths_cache='to',
              assigedIDs_cache='to'):
    """interface.py:170-215: detect growth cones in every frame, then associate them over time."""
    axon_dets_dir = f'{dest_dir}/axon_dets' if dest_dir else None
    if axon_dets_dir is None:
        detections_cache = astar_paths_cache = assigedIDs_cache = None
    axon_detections = AxonDetections(model, timelapse, parameters, axon_dets_dir)
    axon_detections.detect_dataset(cache=detections_cache)
    axon_detections.assign_ids(astar_paths_cache=astar_paths_cache, assigedIDs_cache=assigedIDs_cache)
    return axon_detections
