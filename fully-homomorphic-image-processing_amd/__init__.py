"""MI355X-native BFV ciphertext arithmetic for the homomorphic image circuits of
wfus/Fully-Homomorphic-Image-Processing.  See DESIGN.md.

The package directory name carries hyphens (it mirrors the reference's name), so import it with
    import importlib; fhe = importlib.import_module("fully-homomorphic-image-processing_amd")
or through the `fhip_amd` shim at the repository root.
"""
from . import _lib, circuits, client, parallel, server
from ._lib import FheError, LIB_PATH, HEADER_PATH, HEADER_PATHS
from .keys import Decryptor, DeviceEncryptor, Encryptor, GaloisKeys, KeyGenerator, SeededCiphertexts, SpecialGaloisKeys, SymmetricEncryptor, galois_element
from .client import BatchEncoder
from .circuits import FILTERS, RESAMPLE_CONVENTIONS, RESAMPLE_KERNELS, filter_source_rows, filter_tap_plan, resample_axis_plan, resize_plan
from .evaluator import (FILTER_MAX_TAPS, REMAP_MAX_TAPS, REMAP_MAX_WEIGHTS, REMAP_SKIP, WeightTable, PRESETS, SEED, YQT, Block8x8Plan, DctPlan, Evaluator, FilterPlan, FractionalEncoder, IdctPlan, PlaneMapPlan, PreparedPlain, RotBsgsPlan, RotDiagPlan, RotSumPlan, SEALContext,
                        to_device, to_host)

__all__ = ["KeyGenerator", "GaloisKeys", "SpecialGaloisKeys", "galois_element", "BatchEncoder", "Encryptor", "DeviceEncryptor", "SymmetricEncryptor", "SeededCiphertexts", "Decryptor", "FheError", "LIB_PATH", "HEADER_PATH", "HEADER_PATHS", "PRESETS", "SEED", "YQT", "Block8x8Plan", "PlaneMapPlan", "RotSumPlan", "RotDiagPlan", "RotBsgsPlan", "DctPlan", "IdctPlan", "FilterPlan", "Evaluator",
           "FractionalEncoder", "PreparedPlain", "SEALContext", "to_device", "to_host", "_lib", "parallel", "circuits", "server", "client", "FILTERS", "FILTER_MAX_TAPS", "filter_tap_plan", "filter_source_rows",
           "WeightTable", "REMAP_MAX_TAPS", "REMAP_MAX_WEIGHTS", "REMAP_SKIP", "RESAMPLE_KERNELS", "RESAMPLE_CONVENTIONS", "resample_axis_plan", "resize_plan"]
