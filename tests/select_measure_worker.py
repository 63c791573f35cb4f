"""The child process of tests/test_contraction_select_gpu.py::test_a_measured_choice_goes_to_the_table_once_and_is_reused: python select_measure_worker.py RESULTS.
The tune table is process-wide and read once, so the parent starts this with OSG_TUNE_CACHE = an empty temporary file.  One context with autotune on; each
key of KEYS is launched once through the public entry point (the candidates are timed, the winner stored), then all of them once more (the table answers).
One JSON line per launch: the key, osg_last_route, osg_tune_misses() after it, the lines of the cache file after it, the comparison with float64."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

# osg_gemm 64 x 320 x 1280; the 3 x 3 / stride 1 / pad 1 convolution of one 8 x 8 image, 320 -> 320 channels (the halo kernel and the implicit GEMM compete)
KEYS = [(0, 0, 64, 320, 1280, 1, 1280, 0, 0, 0, 0, 0, 0), (1, 0, 64, 320, 2880, 1, 8, 8, 320, 3, 1, 1, 0)]


def main(results):
    import tuned_rows as tr
    from onnxstream_amd import osgpu
    cache = os.environ["OSG_TUNE_CACHE"]
    assert not os.environ.get("OSG_TUNE_FROZEN") and open(cache).read() == "", "the parent hands over an empty table that may be written"
    gpu = osgpu.Gpu(0)
    gpu._ck(gpu.lib.osg_set_autotune(gpu.ctx, 1))
    # the operands of a key: those of a table row with that key (the row's choice plays no part in the launch)
    cases = [tr.Case(tr.Row(2 * i + 2, *key, 0, 2, 4, 1, 0)) for i, key in enumerate(KEYS)]
    with open(results, "a") as out:
        for launch in (1, 2):
            for key, case in zip(KEYS, cases):
                got, route = case.launch(gpu)
                worst, far = case.compare(got)
                out.write(json.dumps(dict(launch=launch, key=key, route=list(route), misses=int(gpu.lib.osg_tune_misses()), table=open(cache).read().splitlines(),
                                          worst=worst, far=far)) + "\n")
                out.flush()
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
