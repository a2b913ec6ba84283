"""Child program of tests/test_contract_cpu.py: makes every refusal of tests/contract_cases.py against libaxtrack_hip.so in a
process that cannot see a device, then every limit call, and prints one JSON line per call.

    python tests/contract_child.py [--control] [library]     (default: AXT_LIB_PATH, else axtrack_amd/csrc/libaxtrack_hip.so)

The parent starts it with the devices hidden through the environment. Before the first library call it asks the HIP runtime
for the device count, prints it, and stops (exit status 3) unless it is 0: with no device nothing below can launch, so a
refusal that slips past an argument check shows as AXT_EHIP (or 0) instead of running a kernel on out-of-contract arguments.
--control stops after that line, whatever the count (to find out which variable hides the devices on a machine).
Loads the library with ctypes alone: no torch, no axtrack_amd."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contract_cases as cc          # noqa: E402

CTYPES = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double,
          'void': None, 'pointer:char': ctypes.c_char_p}


def device_count():
    """hipGetDeviceCount through ctypes; an error (hipErrorNoDevice) counts as 0 devices."""
    hip = None
    for name in ('libamdhip64.so', 'libamdhip64.so.7', 'libamdhip64.so.6', '/opt/rocm/lib/libamdhip64.so'):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            continue
    if hip is None:
        raise SystemExit('contract_child: cannot load libamdhip64.so')
    n = ctypes.c_int(-1)
    err = hip.hipGetDeviceCount(ctypes.byref(n))
    return (0 if err != 0 else n.value), err


def load(path):
    lib = ctypes.CDLL(path)
    for name, (ret, params) in cc.prototypes().items():
        fn = getattr(lib, name)
        fn.restype = CTYPES.get(ret, ctypes.c_void_p)
        fn.argtypes = [CTYPES.get(c, ctypes.c_void_p) for _, c, _ in params]
    return lib


def main(argv):
    control = '--control' in argv
    argv = [a for a in argv if a != '--control']
    path = argv[0] if argv else os.environ.get('AXT_LIB_PATH') or os.path.join(os.path.dirname(HERE), 'axtrack_amd', 'csrc', 'libaxtrack_hip.so')
    n, err = device_count()
    print(json.dumps({'device_count': n, 'hipGetDeviceCount': err, 'library': path}), flush=True)
    if control:
        return 0
    if n != 0:
        print('contract_child: a device is visible: refusing to send out-of-contract calls', flush=True)
        return 3
    lib = load(path)
    cc.LIB = lib
    sentinel = cc.sentinel_buffer()
    for call in cc.refusals():
        print(json.dumps({'id': call.id, 'begin': True}), flush=True)          # (so that a crash names its call)
        rc, msg, touched = cc.run_refusal(lib, call, sentinel)
        print(json.dumps({'id': call.id, 'function': call.function, 'rc': rc, 'message': msg, 'touched': touched}), flush=True)
    # the limit calls are in the contract: here they must get past every argument check (and then fail at the first HIP call,
    # or succeed where the work is the host's); tests/test_contract_gpu.py runs them on a device
    for call in cc.limits():
        print(json.dumps({'id': call.id, 'begin': True}), flush=True)
        rc, msg, _ = cc.run_refusal(lib, call, sentinel)
        print(json.dumps({'id': call.id, 'function': call.function, 'limit': True, 'rc': rc, 'message': msg}), flush=True)
    print(json.dumps({'done': True}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
