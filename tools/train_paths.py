"""dev tool: the launch sequence of every training path (SwnTrainPath, csrc/swn_train_internal.hpp), for comparing two builds.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/train_paths.py     (nothing else traced)
  python tools/train_paths.py --list DIR/.../t_kernel_trace.csv > listing.txt

The run makes each path's forward and backward once through the C ABI, with the helpers and at the shapes of
tests/test_gpu_train_work_bounds.py (the smallest at which each path is selected).  Ahead of path i it launches a marker:
swn_laplace_head_backward with batch = i + 1 and one position, a kernel no path launches.  --list cuts the trace at the
markers and prints, per path, the ordered (kernel, grid, workgroup, LDS bytes) of the library's launches and the runtime's
fill kernels; torch's own kernels (inputs, guard checks) are left out.  Select the other build's library with SWN_HIP_LIB
and diff the two listings: gradients are not bit-comparable between runs (float atomics), the launches are."""
import csv
import ctypes
import os
import re
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "tests")]


def paths():
    import test_gpu_train_work_bounds as WB
    from shallow_wavenet_amd import config as C
    tiny, ref6, bl6 = C.tiny, C.ref6_laplace, C.bl6_laplace(1, 0)
    return [
        ("fp32_chain", lambda: WB._plain(tiny("laplace", 2, 4), 2, 3, WB.FP32)),
        ("bf16_chain_short", lambda: WB._plain(tiny("laplace", 1, 0), 2, 3, WB.BF16)),
        ("bf16_chain_long", lambda: WB._plain(tiny("laplace", 1, 0), 3, 14, WB.BF16)),
        ("keep_bl6_softmax", lambda: WB._keep(C.bl6_softmax(), 1, 4)),
        ("keep_ref6", lambda: WB._keep(ref6(1, 4), 1, 3)),
        ("compact_bl6", lambda: WB._compact(bl6, 2, 3)),
        ("drop_fp32_seg1", lambda: WB._drop(tiny("laplace", 1, 0), 2, 3, WB.FP32)),
        ("drop_fp32_seg2", lambda: WB._drop(tiny("laplace", 2, 4), 2, 3, WB.FP32)),
        ("drop_bf16_ref6_seg5", lambda: WB._drop(ref6(5, 4), 1, 2, WB.BF16)),
        ("drop_bf16_ref6_stack", lambda: WB._drop(ref6(1, 4), 1, 3, WB.BF16)),
        ("drop_bf16_ref6_own_hs", lambda: WB._drop(ref6(1, 4), 1, 3, WB.BF16, own_hs=True)),
        ("drop_bf16_bl6_fused", lambda: WB._drop(bl6, 2, 3, WB.BF16, masked=[bl6.L - 1], fused=True)),
        ("drop_bf16_bl6_midmask_chain", lambda: WB._drop(bl6, 2, 3, WB.BF16, masked=[2, bl6.L - 1])),
    ]


def run():
    import torch
    from shallow_wavenet_amd import _lib
    from shallow_wavenet_amd import config as C
    from shallow_wavenet_amd.runtime import _ptr, _stream_ptr
    dev = torch.device("cuda:0")
    L, desc = _lib.lib(), _lib.desc_from_cfg(C.tiny("laplace", 1, 0))
    plist = paths()
    raw = torch.zeros((len(plist), 2, 1), dtype=torch.float32, device=dev)      # NO = 2 * seg + lpc = 2
    graw = torch.empty_like(raw)
    for i, (name, fn) in enumerate(plist):
        torch.cuda.synchronize(dev)
        _lib.check(L.swn_laplace_head_backward(ctypes.byref(desc), _ptr(raw), i + 1, 1, None, None, None, None, None, None,
                                               _ptr(graw), _stream_ptr(dev)), "marker")
        fn()
        print(f"{i:2d} {name}: ok", flush=True)


def short(name):
    if name.startswith("_Z"):
        return name
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for k, ch in enumerate(name):             # cut the parameter list, keep the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:k]
    return name


def listing(trace):
    names = [n for n, _ in paths()]
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    field = lambda r, stem: tuple(int(r[f"{stem}_{ax}"]) for ax in "XYZ")
    cur = None
    for r in rows:
        k = short(r["Kernel_Name"])
        if "laplace_head_bwd_kernel" in k:
            cur = field(r, "Grid_Size")[1] - 1
            print(f"== path {cur}: {names[cur]}")
            continue
        if cur is None or re.search(r"\bat::|_ZN2at|rocprim|hipcub|\bc10::", k):
            continue
        lds = r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", "?"))
        print(f"{k}  grid={field(r, 'Grid_Size')} wg={field(r, 'Workgroup_Size')} lds={lds}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        run()
