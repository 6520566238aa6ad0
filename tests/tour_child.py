"""The tour of tests/tour.py in a process of its own (not collected by pytest): tests/test_gpu_clean_memory.py starts it once
per situation, because the library reads FX_DEBUG_FILL once per process and a fresh process is one of the situations.

    python tour_child.py INPUT_DIR SET ORDER OUT.npz

Writes the tour's dict to OUT.npz with np.savez, and beside the results, under "__calls", "__blocks" and "__bytes", the calls
in the order they ran with the totals of fx_debug_fill_info before and after each ([n_calls, 2]), "__byte" the fill value in
force (-1: none) and "__seconds" the wall time of the tour.  Sets nothing in its environment and does not start itself again."""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import tour  # noqa: E402


def main(argv):
    in_dir, which, order, out_path = argv[1:5]
    import pyfastx_amd as fx
    from pyfastx_amd import _lib
    _lib.lib()
    inp = tour.load(in_dir, which)
    log = []
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_path))) as scratch:
        res = tour.run(fx, inp, order, scratch=scratch, probe=_lib.debug_fill_info, log=log)
    seconds = time.perf_counter() - t0
    assert not any(k.startswith("__") for k in res)
    res["__calls"] = np.array([name for name, _, _ in log])
    res["__blocks"] = np.array([[a[1], b[1]] for _, a, b in log], dtype=np.int64)
    res["__bytes"] = np.array([[a[2], b[2]] for _, a, b in log], dtype=np.int64)
    res["__byte"] = np.int64(_lib.debug_fill_info()[0])
    res["__seconds"] = np.float64(seconds)
    with open(out_path, "wb") as f:
        np.savez(f, **res)
    print("tour %s %s: %d arrays of %d calls in %.2f s, fill byte %d, %d blocks filled" % (
        which, order, len(res) - 5, len(log), seconds, int(res["__byte"]), _lib.debug_fill_info()[1]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
