"""Builds fips204_amd/csrc/libmldsa_hip.so (hipcc, --offload-arch=gfx950) in-tree, then the layered libraries, which link the
core and never rebuild it: the pre-hash library fips204_amd/ph/libmldsa_ph.so (include/mldsa_ph.h), the key-deduplication
library fips204_amd/keys/libmldsa_keys.so (include/mldsa_keys.h), the external-mu library fips204_amd/mu/libmldsa_mu.so
(include/mldsa_mu.h), the seed-form key library fips204_amd/seed/libmldsa_seed.so (include/mldsa_seed.h), the strict private-key
import library fips204_amd/keycheck/libmldsa_keycheck.so (include/mldsa_keycheck.h), the mu-stream library
fips204_amd/mus/libmldsa_mus.so (include/mldsa_mus.h), the wire-record library fips204_amd/rec/libmldsa_rec.so (include/mldsa_rec.h)
and the large-batch verify library fips204_amd/vfy/libmldsa_vfy.so (include/mldsa_vfy.h).  Behind them the front layers, built
the same way: the request-signing library fips204_amd/recsign/libmldsa_recsign.so (include/mldsa_recsign.h), whose plan header
includes the wire-record library's (fips204_amd/rec/rec_plan.h).  Last the parse layers: the certificate library
fips204_amd/x509/libmldsa_x509.so (include/mldsa_x509.h), which writes the wire-record library's descriptors and links the core only,
and the issue layers: the certificate-issuing library fips204_amd/x509sign/libmldsa_x509sign.so (include/mldsa_x509sign.h), which
writes the request-signing library's descriptors and links the core only, and the request layers: the certification-request library
fips204_amd/csr/libmldsa_csr.so (include/mldsa_csr.h), which writes the wire-record and the certificate-issuing libraries' descriptors
and links the core only, and the revocation layers: the revocation-list library fips204_amd/crl/libmldsa_crl.so (include/mldsa_crl.h), which
writes the wire-record library's descriptors from CRLs, reads the certificate library's rows and links the core only, and the path layers: the path-validation library
fips204_amd/path/libmldsa_path.so (include/mldsa_path.h), which reads the rows of the certificate and the revocation-list library and
links the core only, and the find layers: the path-building library fips204_amd/find/libmldsa_find.so (include/mldsa_find.h), which reads
the rows of the certificate, the revocation-list and the path-validation library and links the core only."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(CSRC, "libmldsa_hip.so")
# the layered libraries in build order: directory under fips204_amd/ -> library file name
LAYERS = {"ph": "libmldsa_ph.so", "keys": "libmldsa_keys.so", "mu": "libmldsa_mu.so", "seed": "libmldsa_seed.so",
          "keycheck": "libmldsa_keycheck.so", "mus": "libmldsa_mus.so", "rec": "libmldsa_rec.so", "vfy": "libmldsa_vfy.so"}
# built after LAYERS by the same loop
FRONT_LAYERS = {"recsign": "libmldsa_recsign.so"}
# built after FRONT_LAYERS by the same loop
PARSE_LAYERS = {"x509": "libmldsa_x509.so"}
# built after PARSE_LAYERS by the same loop
ISSUE_LAYERS = {"x509sign": "libmldsa_x509sign.so"}
# built after ISSUE_LAYERS by the same loop
REQUEST_LAYERS = {"csr": "libmldsa_csr.so"}
# built after REQUEST_LAYERS by the same loop
REVOCATION_LAYERS = {"crl": "libmldsa_crl.so"}
# built after REVOCATION_LAYERS by the same loop
PATH_LAYERS = {"path": "libmldsa_path.so"}
# built after PATH_LAYERS by the same loop
FIND_LAYERS = {"find": "libmldsa_find.so"}
# PH_DIR, PH_LIB, KEYS_DIR, KEYS_LIB, ... VFY_LIB, RECSIGN_DIR, RECSIGN_LIB, X509_DIR, X509_LIB, X509SIGN_DIR, X509SIGN_LIB, CSR_DIR, CSR_LIB,
# CRL_DIR, CRL_LIB, PATH_DIR, PATH_LIB, FIND_DIR, FIND_LIB
for _name, _file in {**LAYERS, **FRONT_LAYERS, **PARSE_LAYERS, **ISSUE_LAYERS, **REQUEST_LAYERS, **REVOCATION_LAYERS, **PATH_LAYERS, **FIND_LAYERS}.items():
    globals()[f"{_name.upper()}_DIR"] = os.path.join(_HERE, _name)
    globals()[f"{_name.upper()}_LIB"] = os.path.join(_HERE, _name, _file)


def build(force=False, jobs=8):
    args = ["make", "-C", CSRC, f"-j{jobs}"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB):
        raise RuntimeError(f"build did not produce {LIB}")
    for name, file in {**LAYERS, **FRONT_LAYERS, **PARSE_LAYERS, **ISSUE_LAYERS, **REQUEST_LAYERS, **REVOCATION_LAYERS, **PATH_LAYERS, **FIND_LAYERS}.items():
        layer_dir = os.path.join(_HERE, name)
        layer_lib = os.path.join(layer_dir, file)
        if force:
            subprocess.check_call(["make", "-C", layer_dir, "clean"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", layer_dir, f"-j{jobs}"], stdout=subprocess.DEVNULL)
        if not os.path.exists(layer_lib):
            raise RuntimeError(f"build did not produce {layer_lib}")
    return LIB


if __name__ == "__main__":
    print(build())
