"""Child process of test_gpu_first_launch.py: two contexts make their first launches at once.

    python first_launch_child.py DEV_A,DEV_B OUT.npz

A fresh process, so no kernel has been launched and no launch geometry is known anywhere.  Two
threads meet at a barrier; each creates its own Renderer on its device and runs `calls`: the ordered
megakernel with the cost schedule (the pilot's and the LDS kernel's first launch), the same frame on
the wavefront path, one denoise_mix.  Then the same calls run one after the other on fresh contexts.
Everything is written to OUT.npz; the parent asserts.
"""
import sys
import threading

import numpy as np

from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io

NAME, W, H, SPP, DEPTH, SEED = "s4", 64, 40, 2, 32, 1234


def calls(device, before_render=lambda: None):
    cam = camera_get_copy(scenes.camera_for(W, H))
    with Renderer(device) as r:
        r.set_scene(scenes.SCENES[NAME]())
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        r.init_rng(SEED)
        before_render()
        r.render(cam, SPP, DEPTH, aux=True, sync=True, ordered=True, schedule="cost")
        out = {"mk_acc": r.read_accum(), "mk_rng": r.read_rng()}
        r.init_rng(SEED)
        r.render(cam, SPP, DEPTH, aux=True, sync=True, ordered=True, path="wavefront")
        out.update(wf_acc=r.read_accum(), wf_rng=r.read_rng(), bgra=r.denoise_mix(SPP))
    return out


def main():
    import torch  # noqa: F401  (one HIP runtime per process: torch's, as in the suite's `gpu` fixture)
    devices =[int(d) for d in sys.argv[1].split(",")]
    barrier = threading.Barrier(len(devices))
    got, errors = [None] * len(devices), []

    def work(i):
        try:
            barrier.wait(timeout=60)
            got[i] = calls(devices[i], lambda: barrier.wait(timeout=60))
        except BaseException as e:   # noqa: BLE001  (reported by the main thread)
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(devices))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    arrays = {}
    for i, d in enumerate(devices):
        arrays.update({f"thread{i}_{k}": v for k, v in got[i].items()})
        arrays.update({f"seq{i}_{k}": v for k, v in calls(d).items()})
    np.savez(sys.argv[2], **arrays)


if __name__ == "__main__":
    main()
