"""The shapes of tests/test_gpu_distortion_set_scale_n.py: those of tests/probe_set_schedule.py (k_distort_n<true> runs
k_probe_n<true>'s turn loop) and one more at dct_size 9, where a turn holds three blocks; the schedule of a shape under
jpegx_distort_n.hip's own constant.  Nothing of the product is imported."""
import probe_set_schedule as pss

# N -> (the cycle of blocks per plane, planes, the run intended)
SCALE = dict(pss.SCALE)
SCALE[9] = ((4, 1, 7, 2, 3, 11, 1, 5), 5788, 2)          # 3 blocks a turn, 8199 turns


def scale_counts(n):
    cycle, nplanes, _ = SCALE[n]
    return [cycle[p % len(cycle)] for p in range(nplanes)]


def scale_schedule(n):
    return pss.SetSchedule(n, pss.starts_of(scale_counts(n)), pss.constant_of("jpegx_dctn_device.h", "DCTN_THREADS"),
                           pss.constant_of("jpegx_distort_n.hip", "DISTORT_MAX_WORKGROUPS"))
