"""axtrack_amd: AxTrack's detect + associate hot path on AMD Instinct MI355X (gfx950).

Drop-in for the reference's public API on that path (reference __init__.py:1-16):
setup_inference, prepare_input_data, inference -> AxonDetections.IDed_dets_all; PKG_DIR, _compute_astar_path;
visualize_inference exists and says that matplotlib / video plotting is out of scope; render_inference draws the
annotated frames on the GPU and writes PNG frames, one animated PNG, or an MJPEG AVI video whose frames jpeg_encode
compresses on the GPU (jpeg.py; write_mjpeg_avi is the container); segment_mask makes the microchannel mask of
prepare_input_data(mask_fname=...) from a transmission image (data_prep_nbs/00_segment_bg.ipynb); fine_tune_head
trains the detector's three linear layers on labelled frames with the convolutional trunk frozen (training.py), with the
reference's translate / flip / rotate augmentation redrawn every epoch if asked (augment.py); fine_tune_detector trains
any number of the conv blocks with it, down to the whole network; prepare_training_data
makes the labelled train and test timelapses of a recording from its files (core_functionality.setup_data), with the
standardisation scaler measured on the GPU (estimate_stnd_scaler) and the labels read by load_labels_csv; read_tiff reads a
TIFF timelapse without a third-party reader, its strips decoded on the GPU (tiff.py), and every file-name argument takes .tif;
write_tiff writes one as a Deflate TIFF, its strips deflated on the GPU, and process_timelapse is the recording-preparation
step that ends in it (data_prep_nbs/01_process_training_timelapses.ipynb).
The compute lives in csrc/libaxtrack_hip.so (C ABI: include/axtrack_hip.h); there is no CPU
fallback -- importing works anywhere, running needs the GPU and the built library.
"""
from .interface import (setup_inference, prepare_input_data, inference, visualize_inference, prepare_training_data,
                        process_timelapse, PKG_DIR, DEPLOYED_MODEL_DIR)
from .utils import _compute_astar_path
from .detections import AxonDetections
from .hotpath import Detector
from .render import render_inference
from .jpeg import jpeg_encode, write_mjpeg_avi
from .timelapse import Timelapse, estimate_stnd_scaler, load_labels_csv
from .tiff import read_tiff, write_tiff, tiff_info, TiffError, TiffUnsupported
from .training import (ConvBlockTrainer, ConvStageTrainer, ConvTrunkTrainer, HeadTrainer, fine_tune_head, fine_tune_detector,
                       yolo_targets)
from .augment import (Transform, transform_from_uniforms, draw_transform, augment_frames, transform_labels,
                      pos_label_rate)
from .segment import (segment_microchannels, flood_initial_mask, segment_mask, save_final_mask,
                      otsu_threshold_from_hist)

__all__ = ['setup_inference', 'prepare_input_data', 'inference', 'visualize_inference', 'PKG_DIR', 'DEPLOYED_MODEL_DIR',
           '_compute_astar_path', 'AxonDetections', 'Detector', 'Timelapse', 'render_inference', 'jpeg_encode', 'write_mjpeg_avi',
           'ConvBlockTrainer', 'ConvStageTrainer', 'ConvTrunkTrainer', 'HeadTrainer', 'fine_tune_head', 'fine_tune_detector',
           'yolo_targets',
           'prepare_training_data', 'estimate_stnd_scaler', 'load_labels_csv',
           'read_tiff', 'write_tiff', 'process_timelapse', 'tiff_info', 'TiffError', 'TiffUnsupported',
           'Transform', 'transform_from_uniforms', 'draw_transform', 'augment_frames', 'transform_labels', 'pos_label_rate',
           'segment_microchannels', 'flood_initial_mask', 'segment_mask', 'save_final_mask', 'otsu_threshold_from_hist']
