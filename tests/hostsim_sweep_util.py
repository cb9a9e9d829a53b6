"""Builds/loads tests/hostsim/hostsim_sweep.cpp (the sweep chain of closed_form_body.h compiled for the host with g++, the
same command line as hostsim_util).  Test infrastructure."""
import ctypes as C
import os
import subprocess

from neural_inventory_control_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "hostsim_sweep.cpp")
OUT_DIR = os.path.join(HERE, "hostsim", "_build")
OUT = os.path.join(OUT_DIR, "libhostsim_sweep.so")
_h = None


def load():
    global _h
    if _h is not None:
        return _h
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [SRC] + [os.path.join(HERE, "..", "neural_inventory_control_amd", "csrc", f) for f in ("env_step_body.h", "closed_form_body.h")] \
        + [os.path.join(HERE, "..", "include", "nic_rollout.h")]
    if not os.path.isfile(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", OUT])
    h = C.CDLL(OUT)
    vp, i32 = C.c_void_p, C.c_int32
    h.hostsim_closed_form_sweep.argtypes = [C.POINTER(_lib.NicClosedFormDesc), vp, i32, i32, vp, vp]
    h.hostsim_closed_form_sweep.restype = C.c_int
    _h = h
    return h
