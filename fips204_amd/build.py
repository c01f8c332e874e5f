"""Builds fips204_amd/csrc/libmldsa_hip.so (hipcc, --offload-arch=gfx950) in-tree, then the layered libraries, which link the
core and never rebuild it: the pre-hash library fips204_amd/ph/libmldsa_ph.so (include/mldsa_ph.h), the key-deduplication
library fips204_amd/keys/libmldsa_keys.so (include/mldsa_keys.h), the external-mu library fips204_amd/mu/libmldsa_mu.so
(include/mldsa_mu.h), the seed-form key library fips204_amd/seed/libmldsa_seed.so (include/mldsa_seed.h) and the strict private-key
import library fips204_amd/keycheck/libmldsa_keycheck.so (include/mldsa_keycheck.h)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(CSRC, "libmldsa_hip.so")
PH_DIR = os.path.join(_HERE, "ph")
PH_LIB = os.path.join(PH_DIR, "libmldsa_ph.so")
KEYS_DIR = os.path.join(_HERE, "keys")
KEYS_LIB = os.path.join(KEYS_DIR, "libmldsa_keys.so")
MU_DIR = os.path.join(_HERE, "mu")
MU_LIB = os.path.join(MU_DIR, "libmldsa_mu.so")
SEED_DIR = os.path.join(_HERE, "seed")
SEED_LIB = os.path.join(SEED_DIR, "libmldsa_seed.so")
KEYCHECK_DIR = os.path.join(_HERE, "keycheck")
KEYCHECK_LIB = os.path.join(KEYCHECK_DIR, "libmldsa_keycheck.so")


def build(force=False, jobs=8):
    args = ["make", "-C", CSRC, f"-j{jobs}"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB):
        raise RuntimeError(f"build did not produce {LIB}")
    for layer_dir, layer_lib in ((PH_DIR, PH_LIB), (KEYS_DIR, KEYS_LIB), (MU_DIR, MU_LIB), (SEED_DIR, SEED_LIB),
                                 (KEYCHECK_DIR, KEYCHECK_LIB)):
        if force:
            subprocess.check_call(["make", "-C", layer_dir, "clean"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", layer_dir, f"-j{jobs}"], stdout=subprocess.DEVNULL)
        if not os.path.exists(layer_lib):
            raise RuntimeError(f"build did not produce {layer_lib}")
    return LIB


if __name__ == "__main__":
    print(build())
