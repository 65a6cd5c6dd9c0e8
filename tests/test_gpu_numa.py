"""NUMA placement of the host side of a GPU (numa.cpp): the
device's node from sysfs, pinned buffers on that node, thread binding, and a
host batch coded zero-copy from such a buffer (checked against the C oracle)."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _online_nodes():
    try:
        s = open("/sys/devices/system/node/online").read().strip()
    except OSError:
        return 1
    n = 0
    for part in s.split(","):
        a, _, b = part.partition("-")
        n += (int(b) - int(a) + 1) if b else 1
    return n


def test_device_node_and_buffer_placement():
    import torch
    import helyim_amd as H
    torch.cuda.set_device(0)
    node = H.numa_node(0)
    assert node >= -1
    buf = H.HostBuffer(8 << 20)
    buf.array[:] = 1  # resident
    placed = buf.numa_node()
    if node >= 0 and _online_nodes() > 1:
        assert placed == node, f"pinned staging on node {placed}, GPU on node {node}"
    buf.close()


def test_bind_thread_to_device_restricts_affinity():
    import helyim_amd as H
    res = {}

    def work():  # a fresh thread, so the test process keeps its affinity
        before = os.sched_getaffinity(0)
        res["info"] = H.bind_host_to_device(0)
        res["after"] = os.sched_getaffinity(0)
        res["before"] = before

    t = threading.Thread(target=work)
    t.start()
    t.join()
    info = res["info"]
    assert res["after"] <= res["before"]
    if info["bound_cpus"]:
        assert len(res["after"]) == info["bound_cpus"]


def test_host_batch_from_numa_local_buffer():
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    from oracle import corc
    torch.cuda.set_device(0)
    S, L = 6, 65536
    buf = H.HostBuffer(S * 14 * L)
    t = buf.tensor((S, 14, L))
    rng = np.random.default_rng(7)
    t[:, :10] = torch.from_numpy(rng.integers(0, 256, (S, 10, L), dtype=np.uint8))
    rs = H.ReedSolomon(10, 4)
    B.host_encode_batch(rs, t)
    ref = corc.encode_stripes(t[:, :10].numpy().copy())
    assert np.array_equal(t[:, 10:].numpy(), ref)
    good = t.numpy().copy()
    masks = np.full(S, (1 << 14) - 1, np.uint32)
    for s, drop in enumerate([(0, 1, 2, 3), (10, 11, 12, 13), (0, 5, 10, 13), (9,), (4, 12), (1, 6, 11)]):
        for i in drop:
            t[s, i] = 0
            masks[s] &= ~np.uint32(1 << i)
    assert B.host_reconstruct_batch(rs, t, masks) == 0
    assert np.array_equal(t.numpy(), good)
    del t
    buf.close()


_FALLBACK_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import helyim_amd as H, helyim_amd.batch as B
from oracle import corc
torch.cuda.set_device(0)
S, L = 4, 65536
buf = H.HostBuffer(S * 14 * L)          # pinned_alloc with the NUMA-bound attempt failing
t = buf.tensor((S, 14, L))
t[:, :10] = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (S, 10, L), dtype=np.uint8))
rs = H.ReedSolomon(10, 4)
B.host_encode_batch(rs, t)              # zero copy on the fallback buffer
u = torch.zeros((S, 14, L), dtype=torch.uint8)  # pageable: pinned staging slots, also fallback-allocated
u[:, :10] = t[:, :10]
B.host_encode_batch(rs, u)
ref = corc.encode_stripes(t[:, :10].numpy().copy())
assert np.array_equal(t[:, 10:].numpy(), ref) and np.array_equal(u[:, 10:].numpy(), ref)
print("fallback ok")
"""


def test_numa_bound_allocation_falls_back_to_any_node():
    """NUMA placement is speed only. With the bound attempt forced
    to fail (HEC_TEST_NUMA_BIND_FAIL=1, numa.cpp), every pinned buffer libhec
    allocates -- hec_host_alloc and the pipelines' staging -- comes from the
    default policy instead of failing, and the host batches stay bit-exact."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HEC_TEST_NUMA_BIND_FAIL="1")
    p = subprocess.run([sys.executable, "-c", _FALLBACK_CHILD, root], env=env, capture_output=True, text=True,
                       timeout=110, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "fallback ok" in p.stdout


def test_host_buffer_views_keep_the_buffer_alive():
    """a view of a HostBuffer holds the buffer, so dropping the
    HostBuffer object while a view lives does not free the pinned memory."""
    import gc
    import weakref
    import helyim_amd as H
    buf = H.HostBuffer(1 << 20)
    ref = weakref.ref(buf)
    t = buf.tensor((1024, 1024))
    del buf
    gc.collect()
    assert ref() is not None  # still owned by the view
    t[:] = 7                   # writes land in live pinned memory
    assert int(t.sum()) == 7 * (1 << 20)
    del t
    gc.collect()
    assert ref() is None       # freed once the last view is gone


def _allowed_nodes():
    """NUMA nodes this process may allocate on (cgroup cpuset, else online)."""
    for path in ("/sys/fs/cgroup/cpuset.mems.effective", "/sys/devices/system/node/online"):
        try:
            s = open(path).read().strip()
        except OSError:
            continue
        if not s:
            continue
        out = []
        for part in s.split(","):
            a, _, b = part.partition("-")
            out += list(range(int(a), int(b) + 1)) if b else [int(a)]
        return out
    return [0]


def test_multi_device_batch_pages_follow_their_ranges(monkeypatch):
    """VERDICT r03 "next" 4: hec_host_alloc_multi places each _multi stripe
    range's pages on its device's node. The one-GPU box lists device 0
    twice, so a forced node map (HEC_TEST_RANGE_NODES, numa.cpp) stands in for
    two GPUs on two sockets: placement is read back page by page
    (move_pages(.., NULL, status) through hec_host_numa_node), then the batch
    goes through the _multi calls against the C oracle."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    from oracle import corc
    from oracle import rs_oracle as O
    nodes = _allowed_nodes()
    if len(nodes) < 2:
        pytest.skip(f"one NUMA node allowed here ({nodes})")
    a, b = nodes[0], nodes[-1]
    monkeypatch.setenv("HEC_TEST_RANGE_NODES", f"{a},{b}")
    torch.cuda.set_device(0)
    S, L = 10, 1 << 20
    stride = 14 * L
    buf = H.HostBuffer.for_devices([0, 0], stride, S)
    page = os.sysconf("SC_PAGE_SIZE")
    for r, node in ((0, a), (1, b)):
        s0, s1 = S * r // 2, S * (r + 1) // 2
        for off in (s0 * stride, (s0 + s1) // 2 * stride + 12345, s1 * stride - page):
            assert buf.numa_node_at(off) == node, (r, off, buf.numa_node_at(off), node)
    t = buf.tensor((S, 14, L))
    for s in range(S):
        t[s, :10] = torch.from_numpy(corc.splitmix64_bytes(O.STRIPE_SEED_BASE + s, 10 * L).reshape(10, L))
    rs = H.ReedSolomon(10, 4)
    B.host_encode_batch(rs, t, devices=[0, 0])
    want = t.numpy().copy()
    assert np.array_equal(want[:, 10:], corc.encode_stripes(np.ascontiguousarray(want[:, :10])))
    masks = np.full(S, (1 << 14) - 1, np.uint32)
    for s in range(S):
        for i in ((s, 13, 5 + s % 3, 10)[: s % 5]):
            masks[s] &= ~np.uint32(1 << int(i))
            t[s, int(i)] = 0
    assert B.host_reconstruct_batch(rs, t, masks, devices=[0, 0]) == 0
    assert np.array_equal(t.numpy(), want)
    # placement survived the calls (pinned pages do not migrate)
    assert buf.numa_node_at(0) == a and buf.numa_node_at(S * stride - 1) == b
    del t
    buf.close()


def test_host_worker_pool_threads_sit_on_the_gpus_node():
    """Each device's host worker pool binds its workers to that GPU's NUMA
    node (host_pool.cpp HostPool), whichever thread first needed it: after a
    pageable host batch (staging copies on the pool), at least the 15 workers
    of device 0's pool run on exactly the CPUs hec_bind_thread_to_device(0)
    gives a thread here."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    res = {}

    def probe():  # a fresh thread: what binding to device 0 yields here
        res["info"] = H.bind_host_to_device(0)
        res["cpus"] = os.sched_getaffinity(0)

    t = threading.Thread(target=probe)
    t.start()
    t.join()
    if not res["info"]["bound_cpus"] or res["cpus"] == os.sched_getaffinity(0):
        pytest.skip(f"binding to device 0's node changes nothing here ({res['info']})")
    torch.cuda.set_device(0)
    S, L = 16, 1 << 20
    host = torch.zeros((S, 14, L), dtype=torch.uint8)  # pageable: copies on the pool
    host[:, :10] = 7
    B.host_encode_batch(H.ReedSolomon(10, 4), host)
    on_node = 0
    for tid in os.listdir("/proc/self/task"):
        try:
            if os.sched_getaffinity(int(tid)) == res["cpus"]:
                on_node += 1
        except OSError:
            pass
    assert on_node >= 15, (on_node, sorted(res["cpus"])[:8])
