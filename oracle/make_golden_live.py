#!/usr/bin/env python3
"""Golden vectors for the two oracle checks that used to need the reference build next to the tests: the restated
JPEG 2000 encoder against OpenJPEG 2.4.0 on small natural-looking images, and the three EBCC_DISABLE_* switches of the
frame codec.  Generated in the dev container from the REFERENCE build (oracle/_ref/libh5z_ebcc_ref.so) and the oracle's
OpenJPEG backend; TEST INFRASTRUCTURE:

    make -C oracle oracle ref && python3 oracle/make_golden_live.py
        ->  tests/golden/live_checks.json, tests/golden/live_checks_inputs.npz

tests/test_oracle_golden.py::test_j2k_restatement_matches_openjpeg_live and ::test_oracle_env_switches_match_reference
check the oracle against these on any box, and against the libraries themselves where they are.  Inputs are stored,
so the fixtures do not depend on how a numpy build rounds its FFTs."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# the cases of the two tests (tests/test_oracle_golden.py)
OPJ_SIZES = [(32, 32), (45, 70), (100, 130)]
OPJ_CRS = (1.0, 4.0, 17.0, 60.0, 900.0)
ENV_SWITCHES = ["EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK_CONSISTENCY",
                "EBCC_DISABLE_MEAN_ADJUSTMENT"]
ENV_CASES = [("env_a", (1, 64, 96), 25.0, 0.02, L.MAX_ERROR), ("env_a", (1, 64, 96), 8.0, 2e-3, L.RELATIVE_ERROR),
             ("env_b", (1, 96, 64), 40.0, 0.05, L.MAX_ERROR)]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def main():
    lib = L.oracle()
    assert hasattr(lib, "orc_opj_encode") and L.opj_version().startswith("2.4.0"), "needs the OpenJPEG 2.4.0 backend: " + repr(L.opj_version())
    ref = ctypes.CDLL(L.REF_SO)
    ref.ebcc_encode.restype = ctypes.c_size_t
    ref.ebcc_encode.argtypes = [ctypes.c_void_p, ctypes.POINTER(L.CodecConfig), L.c_void_pp]

    def opj(img, cr):
        out = ctypes.c_void_p()
        n = lib.orc_opj_encode(img.ctypes.data, img.shape[0], img.shape[1], ctypes.c_float(cr), ctypes.byref(out))
        s = ctypes.string_at(out.value, n)
        lib.orc_free(out)
        return s

    arrays = {}
    opj_cases = []
    for h, w in OPJ_SIZES:
        f = L.era5_like(h, w, h + w)
        name = f"opj_{h}x{w}"
        arrays[name] = np.ascontiguousarray((((f - f.min()) / (f.max() - f.min())) * np.float32(65535)).astype(np.uint16))
        for cr in OPJ_CRS:
            s = opj(arrays[name], cr)
            opj_cases.append({"input": name, "cr": cr, "n": len(s), "stream_sha256": sha(s)})

    arrays["env_a"] = np.ascontiguousarray(L.era5_like(64, 96, 21, 1.0, 0.8), np.float32)
    arrays["env_b"] = np.ascontiguousarray(L.smooth_image(96, 64, 5), np.float32)
    env = {}
    os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = "0.1"              # loose base layer: the switches change the streams
    for switch in ENV_SWITCHES:
        os.environ[switch] = "1"
        env[switch] = []
        for name, shape, cr, err, mode in ENV_CASES:
            cfg = L.make_config(shape, base_cr=cr, error=err, residual_type=mode)
            out = ctypes.c_void_p()
            n = ref.ebcc_encode(arrays[name].ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
            s = ctypes.string_at(out.value, n)
            env[switch].append({"input": name, "shape": list(shape), "base_cr": cr, "error": err, "mode": mode,
                                "n": len(s), "stream_sha256": sha(s)})
        del os.environ[switch]

    np.savez_compressed(os.path.join(OUT, "live_checks_inputs.npz"), **arrays)
    json.dump({"openjpeg": L.opj_version(), "opj": opj_cases, "env_quantile": "0.1", "env_switches": env},
              open(os.path.join(OUT, "live_checks.json"), "w"), indent=0)
    print(len(opj_cases), "OpenJPEG cases,", sum(len(v) for v in env.values()), "switch cases")


if __name__ == "__main__":
    main()
