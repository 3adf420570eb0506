"""How many GPUs the installed HIP runtime sees (hipGetDeviceCount of libamdhip64): the tests meant for machines without a
GPU skip themselves where this is not 0.  PyTorch is no witness for it: its wheel carries a HIP runtime of its own, which
need not see the device that the runtime the library links against does."""
import ctypes as C
import os


def visible_gpus():
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for name in ('libamdhip64.so', os.path.join(rocm, 'lib', 'libamdhip64.so')):
        try:
            hip = C.CDLL(name)
        except OSError:
            continue
        n = C.c_int(0)
        return n.value if hip.hipGetDeviceCount(C.byref(n)) == 0 else 0
    return 0
