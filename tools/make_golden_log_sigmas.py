"""Generate tests/golden/log_sigmas.npz: the 1000 log-sigma literals of the reference application's table (src/sd.cpp, `float const
log_sigmas[1000]`), parsed as the compiler reads them (decimal -> float32).  DATA only: the bit-for-bit sampler tests of tests/test_pipeline.py
drive the harness with these literals instead of the recomputed table (pipeline.log_sigmas_table), without needing the reference sources."""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference/src")


def parse(src: str) -> np.ndarray:
    i = src.index("float const log_sigmas[1000] = {")
    body = src[i:src.index("};", i)].split("{")[1]
    return np.asarray([float(x.strip().rstrip("f")) for x in body.split(",")], np.float64).astype(np.float32)


if __name__ == "__main__":
    t = parse(open(os.path.join(REF, "sd.cpp")).read())
    assert t.shape == (1000,)
    out = os.path.join(REPO, "tests", "golden", "log_sigmas.npz")
    np.savez_compressed(out, log_sigmas=t)
    print(out, t.shape, t.dtype)
