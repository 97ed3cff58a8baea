#!/usr/bin/env python3
"""Mint tests/golden/blake3_vectors.json: Blake3 digests (default hash mode, 32 bytes) from the reference's portable C implementation.

Python's hashlib has Blake2s but no Blake3, so the ground truth of tests/blake_model.py's Blake3 is the reference's CPU code
(backend/cpu/src/hash/blake3.c, blake3_dispatch.c, blake3_portable.c), compiled in place with every SIMD path disabled into a
temporary directory that is deleted afterwards. Only data is recorded: message length -> hex digest for the input pattern of the
published BLAKE3 test vectors (byte i = i % 251), and the known-answer message of the reference's own test
(icicle/tests/test_hash_api.cpp:105-108). Needs the reference tree ($ICICLE_REFERENCE_DIR, default /root/reference) and gcc; the
tests read only the JSON.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle", "backend", "cpu", "src", "hash")
FLAGS = ["-DBLAKE3_NO_SSE2", "-DBLAKE3_NO_SSE41", "-DBLAKE3_NO_AVX2", "-DBLAKE3_NO_AVX512", "-DBLAKE3_USE_NEON=0"]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 7168, 7169, 8192, 8193,
           9216, 16384, 16385]
KNOWN_ANSWER_MESSAGE = ("Hello world I am blake3. This is a semi-long C++ test with a lot of characters. "
                        "0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef")


def main():
    sources = [os.path.join(SRC, f) for f in ("blake3.c", "blake3_dispatch.c", "blake3_portable.c")]
    missing = [s for s in sources if not os.path.exists(s)]
    if missing:
        sys.exit(f"reference tree not found ({missing[0]}): nothing minted")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libblake3_portable.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", *FLAGS, *sources, "-o", so])
        lib = ctypes.CDLL(so)
        for fn in (lib.blake3_hasher_init, lib.blake3_hasher_update, lib.blake3_hasher_finalize):
            fn.restype = None
        lib.blake3_hasher_update.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.blake3_hasher_finalize.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.blake3_hasher_init.argtypes = [ctypes.c_void_p]

        def blake3(msg: bytes) -> str:
            state = ctypes.create_string_buffer(4096)  # blake3_hasher is under 2 KiB
            out = ctypes.create_string_buffer(32)
            lib.blake3_hasher_init(state)
            lib.blake3_hasher_update(state, msg, len(msg))
            lib.blake3_hasher_finalize(state, out, 32)
            return out.raw.hex()

        doc = {
            "input": "byte i of a message is i % 251",
            "by_length": {str(n): blake3(bytes(i % 251 for i in range(n))) for n in LENGTHS},
            "known_answer": {"message": KNOWN_ANSWER_MESSAGE, "digest": blake3(KNOWN_ANSWER_MESSAGE.encode())},
        }
        del lib
    with open(os.path.join(HERE, "blake3_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(doc['by_length'])} lengths and the known answer written")


if __name__ == "__main__":
    main()
