"""soundchunks_amd: MI355X-native SoundChunks encode hot path.

Reference: GliGli's SoundChunks encoder (bravesoftdz/soundchunks), whose
per-frame vector quantisation (yakmo k-means++ + KNNScanReduce over ANN's
kd-tree, then the KNNFit nearest-chunk search) runs here as hand-written
gfx950 HIP kernels behind the extern.pas C ABI (include/soundchunks.h).
``Decoder`` reads a ``.gsc`` back to PCM (decoder/decoder.lpr) on the same device.
"""
from .encoder import Encoder, encode_many, frame_dsp, knnfit_assign, knnfit_assign_many, parse_options, scan_reduce, set_device, yakmo_seed_means, yakmo_seed_means_many  # noqa: F401
from .decoder import CropBinding, Decoder, Envelope, Fidelity, Index, ResidentStream, StreamSet  # noqa: F401
from ._lib import GscError, LIB_PATH, load  # noqa: F401

__all__ = ["Decoder", "Index", "ResidentStream", "StreamSet", "CropBinding", "Envelope", "Fidelity", "Encoder", "encode_many", "frame_dsp", "parse_options", "set_device", "yakmo_seed_means", "yakmo_seed_means_many", "scan_reduce", "knnfit_assign", "knnfit_assign_many", "GscError", "load",
           "LIB_PATH"]
