"""sr_mi355x -- MI355X-native multi-frame super-resolution core (libsrx.so + host shim).

Mirrors the call surface of the reference's SR core (mono_cal_target/run_sr.py:157-209):
blur, forward_model, back_project, shift_and_add, ibp (+ ndi_zoom / ndi_shift), see api.py.
Attributes are resolved lazily so that `sr_mi355x.synth` (numpy only) imports without torch.
"""
import importlib

_API = ("blur", "forward_model", "back_project", "shift_and_add", "ibp", "ndi_zoom", "ndi_shift",
        "blur_batched", "shift_batched", "zoom_batched", "forward_model_batched", "back_project_batched",
        "shift_and_add_batched", "ibp_batched", "shift_and_add_u8_batched", "ibp_u8_batched", "decimate_u8", "extract_red_u8", "decimate", "extract_red", "zero_insert", "mean_frames", "mean_frames_batched", "mean_u8", "png_deflate", "png_encode", "png_file", "crc32",
        "bayer_split", "bayer_mean_u8", "bayer_merge", "png_file_rgb8",
        "quantize_u8", "u8_to_float", "interleave4", "make_gaussian_psf", "set_precision", "get_precision", "precision_override", "last_path",
        "FLAG_AUTO", "FLAG_COMPOSED", "FLAG_FUSED", "FLAG_PER_FRAME", "FLAG_TILES", "FLAG_DIAG_NO_ZERO_FUSE",
        "FLAG_DIAG_NO_SEPARABLE", "FLAG_DIAG_NO_PREFILTER_TILE", "FLAG_DIAG_V1", "FLAG_DIAG_WIDE_WINDOWS", "FLAG_DIAG_COLUMN_TILES", "FLAG_DIAG_TWO_LAUNCH", "FLAG_DIAG_SAA_ONE_PASS", "FLAG_DIAG_U8_BYTE_LOADS")

_PATCHWISE = ("PatchGrid", "estimate_shift_field", "reconstruct_patchwise")
__all__ = list(_API) + ["estimate_shifts", "estimate_psf"] + list(_PATCHWISE)


def __getattr__(name):
    if name in _API:
        return getattr(importlib.import_module(".api", __name__), name)
    if name == "estimate_shifts":
        return importlib.import_module(".register", __name__).estimate_shifts
    if name == "estimate_psf":
        return importlib.import_module(".psf_device", __name__).estimate_psf
    if name in _PATCHWISE:  # (patchwise.gather / patchwise.blend stay in their module: the names are too plain for the package)
        return getattr(importlib.import_module(".patchwise", __name__), name)
    if name in ("api", "synth", "_lib", "session", "parallel", "rowband", "metrics", "register", "psf_device", "patchwise"):
        return importlib.import_module("." + name, __name__)
    raise AttributeError(name)
