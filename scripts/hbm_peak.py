"""Practical HBM rates on this device (torch copy / read-reduce / fill), for context next to the 8 TB/s nominal peak."""
import time  # noqa: F401

import torch

N_FLOATS = 2 * 1024**3  # floats: 8 GiB


def t(f, reps=10):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def copy_rate(dev=None, n=N_FLOATS, reps=10):
    """Bytes read + written per second by a torch copy of n floats (the first leg below); other scripts quote
    their rates as fractions of this one, measured in their own session."""
    dev = dev or torch.device("cuda:0")
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    dt = t(lambda: b.copy_(a), reps)
    return 2 * n * 4 / dt


def main():
    dev = torch.device("cuda:0")
    n = N_FLOATS
    print("copy   (R+W) %.2f TB/s" % (copy_rate(dev, n) / 1e12))
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    dt = t(lambda: a.sum());    print("reduce (R)   %.2f TB/s" % (n * 4 / dt / 1e12))
    dt = t(lambda: b.zero_());  print("fill   (W)   %.2f TB/s" % (n * 4 / dt / 1e12))
    dt = t(lambda: torch.add(a, 1.0, out=b)); print("add    (R+W) %.2f TB/s" % (2 * n * 4 / dt / 1e12))


if __name__ == "__main__":
    main()
