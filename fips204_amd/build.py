"""Builds fips204_amd/csrc/libmldsa_hip.so (hipcc, --offload-arch=gfx950) in-tree, then the layered pre-hash library
fips204_amd/ph/libmldsa_ph.so (include/mldsa_ph.h), which links the core and never rebuilds it."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libmldsa_hip.so")
PH_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ph")
PH_LIB = os.path.join(PH_DIR, "libmldsa_ph.so")


def build(force=False, jobs=8):
    args = ["make", "-C", CSRC, f"-j{jobs}"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB):
        raise RuntimeError(f"build did not produce {LIB}")
    if force:
        subprocess.check_call(["make", "-C", PH_DIR, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", PH_DIR, f"-j{jobs}"], stdout=subprocess.DEVNULL)
    if not os.path.exists(PH_LIB):
        raise RuntimeError(f"build did not produce {PH_LIB}")
    return LIB


if __name__ == "__main__":
    print(build())
