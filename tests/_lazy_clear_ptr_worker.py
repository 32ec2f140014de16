"""Child process of test_lazy_clear_gpu.test_pointer_handed_out: reads the accumulators through a torch tensor over
f2q_counts_device_ptr.  A process of its own because torch brings its own HIP runtime: it is initialised first, as
bench.py does, and never inside the pytest process, where the product's library is already loaded.  Prints one JSON
line: the device vector (counts then the five statistics) at each point of the scenario."""
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = importlib.import_module("2fast2q_amd")
    lib = P.binding.synth_library(0xD1E7, 2000, 20)
    out = {}
    with P.Counter(features=lib, miss=1, phred=30, length=20, start="0") as c:
        a = bytes(c.synth_fastq(seed=46, n_reads=17 * 256, read_len=150))
        c.count_block(a)
        c.reset()                                           # a pending clear when the pointer is handed out
        ptr, n64 = c.counts_device_ptr()

        class _Arr:
            __cuda_array_interface__ = {"shape": (n64,), "typestr": "<i8", "data": (ptr, False), "version": 3}
        acc = torch.as_tensor(_Arr(), device=dev)
        stream = torch.cuda.ExternalStream(c.stream(), device=dev)

        def device_vector():
            stream.synchronize()
            return acc.cpu().tolist()
        out["n64"] = n64
        out["handed_out"] = device_vector()
        c.count_block(a)
        out["counted"] = device_vector()
        c.reset()                                           # no further call of the library before the read
        out["reset"] = device_vector()
        counts, stats = c.read_counts()
        out["reset_read_counts"] = [int(v) for v in counts] + [int(v) for v in stats]
        c.count_block(a)
        out["counted_again"] = device_vector()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
