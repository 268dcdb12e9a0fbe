"""The kernels a stack pass enqueues, in enqueue order (run on the GPU box):
    rocprofv3 --kernel-trace --stats -d DIR -o seq --output-format csv -- python tools/pass_sequence.py run
    python tools/pass_sequence.py list DIR > profiles/<name>.txt
`run`: two passes each, on one handle each, of sigma 128 frames, winsorized 24 and winsorized 300 on a 512-row tile; then
a group of three 256-row tiles on device 0, sigma 300 frames: one default pass and one maps pass on the deep tier; then one
pass each on a 64-row tile of the full maps tier (sigma 24 and 300 frames, MAD sigma 24 and 120), the resident maps tier
(linear fit 24) and the three weighted entries (24 and 200 frames).
`list`: kernel name, grid and workgroup size and queue (numbered by first appearance) of every dispatch of the trace,
in dispatch order -- two libraries that enqueue the same work in the same order give the same listing."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if sys.argv[1] == "run":
    from nightlight_amd import StackGroup, StackHandle
    for mode, n in ((2, 128), (3, 24), (3, 300)):
        with StackHandle(n, 4096, 4096, device=0, row0=1536, rows=512) as st:
            st.fill_synthetic(seed=1)
            for _ in range(2):
                st.run(mode, 3.0, 3.0, fetch=False)
    with StackGroup(300, 4096, 768, devices=[0, 0, 0]) as g:
        g.fill_synthetic(seed=1)
        g.run(2, 3.0, 3.0, download=False)
        g.run_maps_deep(2, 3.0, 3.0)
    # one small leg per launch path that takes an nl::Form (a 4096 x 64-row tile): the maps tiers, the weighted entries
    import numpy as np

    def tile(n):
        st = StackHandle(n, 4096, 4096, device=0, row0=1536, rows=64)
        st.fill_synthetic(seed=1)
        return st
    for mode, depths in ((2, (24, 300)), (4, (24, 120))):
        for n in depths:
            with tile(n) as st:
                st.run_maps_full(mode, 3.0, 3.0)
    with tile(24) as st:
        st.run_maps_resident(5, 3.0, 3.0)
    for n in (24, 200):
        with tile(n) as st:
            st.set_weights(np.linspace(0.5, 1.5, n, dtype=np.float32))
            st.run_linfit_weighted(3.0, 3.0, fetch=False)
            st.run_clip_weighted(2, 3.0, 3.0, fetch=False)
            st.run_mad_weighted(3.0, 3.0, fetch=False)
else:
    path, = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    queues = {}
    for r in rows:
        q = queues.setdefault(r["Queue_Id"], len(queues))
        print("q%d  grid %8d  wg %4d  %s" % (q, int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]), r["Kernel_Name"]))
