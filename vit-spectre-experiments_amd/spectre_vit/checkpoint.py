"""Full-state checkpoints of a training run and what a bit-exact resume needs.

Everything a step changes lives on the device -- weights, moments, averages, the optimizer's step count and 64-byte control block, the
accumulators of an open window, the resident loader's cursor, the graphed step's seed word -- so a checkpoint is taken THERE:

    snap = StateSnapshot(named_blocks, out_dir, gated=names)        # once per run; the blocks' addresses are fixed
    snap.take(host_part, epoch)                                     # ONE spv_snapshot_multi launch, in stream order; returns at once
    snap.close()                                                    # joins the writer

``take`` copies every block into its slot of one flat staging buffer (and forms, in the same launch, the per-chunk checksums and the
counts of non-finite fp32 values), records an event, enqueues ONE device-to-host copy of staging + partials on a side stream behind
that event and hands a writer thread the rest: wait for the copy, fold the partials, write ``train_state.pt.tmp``, ``os.fsync``,
``os.replace``.  Training goes on at once: the live tensors are no longer needed.  A killed process leaves the old file whole; a
non-finite value in a gated block (a model parameter or an average) leaves the old file too and yields a ``CheckpointSkipped`` record.

The file (format version 1): the 8 magic bytes, the version, the header's length and checksum, the header -- a pickled dict of the
host part and, per job, name / dtype / shape / byte count / checksum / offset -- and the payload, the staging buffer's slots as they
were laid out (256-byte aligned).  ``load_train_state`` recomputes every job's checksum with numpy and refuses a mismatch, an unknown
version or a truncated file with a ``ValueError`` that names the job.

The checksum of a block: the sum, mod 2^64, of its bytes read as little-endian 32-bit words, the last partial word zero-padded
(``checksum32``).  Integer addition makes it independent of the chunking.
"""
from __future__ import annotations

import os
import pickle
import queue
import struct
import threading
import time

import numpy as np
import torch

FORMAT_VERSION = 1
FILE_NAME = "train_state.pt"
MAGIC = b"SPVSTATE"
SLOT_ALIGN = 256
CHUNK_BYTES = 1 << 16   # 256 lanes x 16 bytes x 16 rounds per workgroup; the Small model's 52 MB of state make ~1000 workgroups
_PREAMBLE = "<8sIQQ"    # magic, version, header bytes, header checksum
_MASK = (1 << 64) - 1


# ---------------------------------------------------------------- pure host functions
def plan_chunks(sizes, chunk_bytes):
    """the chunk table of spv_snapshot_multi for jobs of `sizes` bytes -> (chunk_job, chunk_off): chunk c is bytes
    [chunk_off[c], min(chunk_off[c] + chunk_bytes, size)) of job chunk_job[c].  Every byte of every job is in exactly one chunk, the
    offsets are multiples of 16 (chunk_bytes is one), a job of 0 bytes has no chunk."""
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes <= 0 or chunk_bytes % 16:
        raise ValueError(f"chunk_bytes={chunk_bytes} must be a positive multiple of 16")
    chunk_job, chunk_off = [], []
    for j, size in enumerate(sizes):
        size = int(size)
        if size < 0:
            raise ValueError(f"job {j}: {size} bytes")
        for off in range(0, size, chunk_bytes):
            chunk_job.append(j)
            chunk_off.append(off)
    return chunk_job, chunk_off


def plan_slots(sizes, align=SLOT_ALIGN):
    """-> (the slots' offsets in the staging buffer, each a multiple of `align`; the buffer's length, a multiple of `align`)"""
    offsets, end = [], 0
    for size in sizes:
        offsets.append(end)
        end += -(-int(size) // align) * align
    return offsets, end


def checksum32(data):
    """the sum, mod 2^64, of `data` (bytes, or anything numpy takes as a buffer of bytes) read as little-endian 32-bit words, the last
    partial word zero-padded"""
    b = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    whole = b.size // 4 * 4
    total = int(b[:whole].view("<u4").sum(dtype=np.uint64)) if whole else 0
    for i, byte in enumerate(b[whole:].tolist()):
        total += byte << (8 * i)
    return total & _MASK


def fold_partials(chunk_job, chunk_sum, chunk_nonfinite, njobs):
    """the kernel's per-chunk partials -> per job (checksum, non-finite count)"""
    sums, bad = [0] * njobs, [0] * njobs
    for j, s, n in zip(chunk_job, chunk_sum, chunk_nonfinite):
        sums[j] = (sums[j] + int(s)) & _MASK
        bad[j] += int(n)
    return sums, bad


def check_fingerprint(saved, mine):
    """a resume continues the run that was saved: raises a ValueError that names the first differing key"""
    for k in list(mine) + [k for k in saved if k not in mine]:
        if k not in saved or k not in mine or saved[k] != mine[k]:
            raise ValueError(f"resume: the saved run's fingerprint differs in {k!r}: {saved.get(k, '<absent>')!r} in the file, "
                             f"{mine.get(k, '<absent>')!r} in this call")


def _dtype_name(dtype):
    return str(dtype).replace("torch.", "")


def host_rng_state(gen=None):
    """the host's and the device's generator states, as the objects their setters take"""
    import random
    st = {"torch": torch.get_rng_state(), "python": random.getstate(), "numpy": np.random.get_state()}
    if torch.cuda.is_available():
        st["cuda"] = torch.cuda.get_rng_state_all()
    if gen is not None:
        st["gen"] = gen.get_state()
    return st


def set_host_rng_state(st, gen=None):
    import random
    torch.set_rng_state(st["torch"])
    random.setstate(st["python"])
    np.random.set_state(st["numpy"])
    if "cuda" in st and torch.cuda.is_available():
        torch.cuda.set_rng_state_all(st["cuda"])
    if gen is not None and "gen" in st:
        gen.set_state(st["gen"])


# ---------------------------------------------------------------- the file
def _write_file(path, host_part, metas, payload):
    """header + payload -> path + ".tmp", flushed to the disk, then moved over `path` in one step"""
    header = pickle.dumps({"version": FORMAT_VERSION, "host": host_part, "jobs": metas}, protocol=pickle.HIGHEST_PROTOCOL)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(struct.pack(_PREAMBLE, MAGIC, FORMAT_VERSION, len(header), checksum32(header)))
        f.write(header)
        f.write(payload)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    return struct.calcsize(_PREAMBLE) + len(header) + len(payload)


def commit(path, host_part, metas, payload, sums, nonfinite, gated, epoch):
    """the writer's last step, with every job's checksum and non-finite count known: the gate, then the file.  metas: per job a dict
    of name / dtype / shape / bytes / offset; payload: the slots (a buffer of bytes).  -> {"Checkpoint": {...}} with the file's
    bytes, or {"CheckpointSkipped": {...}} -- the old file untouched -- when a gated job holds a non-finite value"""
    for m, bad in zip(metas, nonfinite):
        if bad and m["name"] in gated:
            return {"CheckpointSkipped": {"epoch": epoch, "job": m["name"], "nonfinite": int(bad)}}
    metas = [dict(m, checksum=int(s)) for m, s in zip(metas, sums)]
    return {"Checkpoint": {"epoch": epoch, "bytes": _write_file(path, host_part, metas, payload)}}


def write_train_state(path, host_part, named_tensors, gated=(), epoch=0):
    """the host-side form of a checkpoint, for tensors that live on the HOST (tools, tests of the format): the same layout, checksum
    definition, gate and file as StateSnapshot.take -- no device, no kernel.  -> commit()'s record"""
    named = [(n, t.detach().contiguous()) for n, t in named_tensors]
    raws = [t.reshape(-1).view(torch.uint8).numpy() for _, t in named]
    offsets, total = plan_slots([r.size for r in raws])
    payload = np.zeros(total, dtype=np.uint8)
    metas, sums, bad = [], [], []
    for (name, t), raw, off in zip(named, raws, offsets):
        payload[off:off + raw.size] = raw
        metas.append(dict(name=name, dtype=_dtype_name(t.dtype), shape=tuple(t.shape), bytes=int(raw.size), offset=off))
        sums.append(checksum32(raw))
        words = raw[:raw.size // 4 * 4].view("<u4")
        bad.append(int(((words & 0x7F800000) == 0x7F800000).sum()) if t.dtype == torch.float32 else 0)
    return commit(path, host_part, metas, memoryview(payload), sums, bad, frozenset(gated), epoch)


def load_train_state(path, fingerprint=None):
    """-> {"version", "host", "tensors": name -> CPU tensor, "jobs": the per-job records}.  Every job's checksum is recomputed on the
    host; a mismatch, an unknown version or a truncated file raises a ValueError that names the job (or the header).  fingerprint:
    this call's, held against the file's (check_fingerprint)."""
    with open(path, "rb") as f:
        data = f.read()
    n0 = struct.calcsize(_PREAMBLE)
    if len(data) < n0:
        raise ValueError(f"{path}: truncated in its preamble ({len(data)} bytes)")
    magic, version, hlen, hsum = struct.unpack(_PREAMBLE, data[:n0])
    if magic != MAGIC:
        raise ValueError(f"{path}: not a train-state file (magic {magic!r})")
    if version != FORMAT_VERSION:
        raise ValueError(f"{path}: unknown format version {version} (this build reads version {FORMAT_VERSION})")
    if len(data) < n0 + hlen:
        raise ValueError(f"{path}: truncated in its header")
    if checksum32(data[n0:n0 + hlen]) != hsum:
        raise ValueError(f"{path}: the header's checksum does not match")
    header = pickle.loads(data[n0:n0 + hlen])
    if header.get("version") != FORMAT_VERSION:
        raise ValueError(f"{path}: unknown format version {header.get('version')} in the header")
    payload = np.frombuffer(data, dtype=np.uint8, offset=n0 + hlen)
    tensors = {}
    for m in header["jobs"]:
        lo, hi = m["offset"], m["offset"] + m["bytes"]
        if hi > payload.size:
            raise ValueError(f"{path}: truncated inside job {m['name']!r} ({max(payload.size - lo, 0)} of {m['bytes']} bytes)")
        raw = payload[lo:hi]
        got = checksum32(raw)
        if got != m["checksum"]:
            raise ValueError(f"{path}: job {m['name']!r}: checksum {got:#018x} differs from the saved {m['checksum']:#018x}")
        t = torch.from_numpy(raw.copy())
        tensors[m["name"]] = t.view(getattr(torch, m["dtype"])).reshape(m["shape"]) if m["bytes"] else \
            torch.empty(m["shape"], dtype=getattr(torch, m["dtype"]))
    if fingerprint is not None:
        check_fingerprint(header["host"].get("fingerprint", {}), fingerprint)
    return {"version": version, "host": header["host"], "tensors": tensors, "jobs": header["jobs"]}


# ---------------------------------------------------------------- an optimizer's state as blocks
def optimizer_blocks(optimizer):
    """an optimizer's per-parameter state in torch's state_dict numbering, split by where it lives -> (blocks, host_state, aliases):
    blocks      [(name, device tensor)], name "optim/<parameter index>/<key>"; a tensor shared by several entries (the fused
                optimizers' one step count per group) appears once
    host_state  {index: {key: value}} for what lives on the host (torch.optim.AdamW's eager ``step``) or is no tensor
    aliases     {(index, key): the block's name that holds the shared tensor}
    No device read, no synchronisation."""
    blocks, host_state, aliases, seen = [], {}, {}, {}
    idx = 0
    for group in optimizer.param_groups:
        for p in group["params"]:
            for key, v in optimizer.state.get(p, {}).items():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    ident = (v.data_ptr(), v.numel(), v.dtype)
                    if v.numel() and ident in seen:
                        aliases[(idx, key)] = seen[ident]
                        continue
                    name = f"optim/{idx}/{key}"
                    seen[ident] = name
                    blocks.append((name, v))
                elif v is not None:
                    host_state.setdefault(idx, {})[key] = v.clone() if isinstance(v, torch.Tensor) else v
            idx += 1
    return blocks, host_state, aliases


def packed_param_groups(optimizer):
    """``param_groups`` as torch's state_dict() packs them (the hyper-parameters, parameters as indices), without reading the device"""
    out, idx = [], 0
    for g in optimizer.param_groups:
        d = {k: v for k, v in g.items() if k != "params"}
        d["params"] = list(range(idx, idx + len(g["params"])))
        idx += len(g["params"])
        out.append(d)
    return out


def optimizer_state_dict(tensors, host):
    """a loaded file -> the optimizer state_dict (torch's layout) that optimizer_blocks / packed_param_groups were saved from"""
    state = {}
    for name, t in tensors.items():
        parts = name.split("/", 2)
        if len(parts) == 3 and parts[0] == "optim" and parts[1].isdigit():   # (not the control block, not the accumulators)
            state.setdefault(int(parts[1]), {})[parts[2]] = t
    for (idx, key), name in host.get("optim_aliases", {}).items():
        state.setdefault(idx, {})[key] = tensors[name]
    for idx, entries in host.get("optim_host", {}).items():
        state.setdefault(idx, {}).update(entries)
    return {"state": state, "param_groups": host["param_groups"]}


# ---------------------------------------------------------------- the device side
class _Writer:
    """one thread, one job at a time: the wait for the device-to-host copy, the fold and the file happen behind the training's back"""

    def __init__(self):
        self._jobs = queue.Queue()
        self._pending = False
        self._done = threading.Event()
        self._result = None
        self._thread = threading.Thread(target=self._loop, name="spv-checkpoint-writer", daemon=True)
        self._thread.start()

    def _loop(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            try:
                self._result = job()
            except BaseException as e:   # handed to the training thread at its next wait()
                self._result = e
            self._done.set()

    def submit(self, job):
        assert not self._pending
        self._done.clear()
        self._pending = True
        self._jobs.put(job)

    def wait(self):
        """-> (the finished job's result or None when none was pending, the milliseconds waited); a job's exception is raised here"""
        if not self._pending:
            return None, 0.0
        t0 = time.perf_counter()
        self._done.wait()
        self._pending = False
        result, self._result = self._result, None
        if isinstance(result, BaseException):
            raise RuntimeError(f"the checkpoint writer failed: {result!r}") from result
        return result, (time.perf_counter() - t0) * 1e3

    def close(self):
        try:
            return self.wait()
        finally:
            if self._thread.is_alive():
                self._jobs.put(None)
                self._thread.join()


class StateSnapshot:
    """named_blocks: [(name, device tensor)], contiguous, at addresses that stay fixed for the run.  gated: the names whose non-finite
    count keeps a checkpoint from being written (model parameters, averages; moments and accumulators are NOT gated: an open window may
    hold an inf that its boundary will drop).  report(record): called on the training thread with every finished write's record
    ({"Checkpoint": {"epoch", "bytes", "take_ms", "wait_ms", "write_ms"}} or {"CheckpointSkipped": ...}) -- at the next take() or at
    close().  ONE staging buffer on the device (slots, then the two partial arrays) and ONE pinned host buffer of the same size."""

    def __init__(self, named_blocks, out_dir, gated=(), report=None, chunk_bytes=CHUNK_BYTES):
        from spectre_vit import _native
        named_blocks = list(named_blocks)
        if not named_blocks:
            raise ValueError("StateSnapshot: no blocks")
        names = [n for n, _ in named_blocks]
        if len(set(names)) != len(names):
            raise ValueError("StateSnapshot: block names must be unique")
        for name, t in named_blocks:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"StateSnapshot: block {name!r} must be a contiguous tensor on the GPU")
        self.path = os.path.join(out_dir, FILE_NAME)
        self.gated = frozenset(gated)
        self.report = report
        self.chunk_bytes = int(chunk_bytes)
        self._blocks = [t for _, t in named_blocks]   # kept alive: the job table holds their addresses
        dev = self._blocks[0].device
        sizes = [t.numel() * t.element_size() for t in self._blocks]
        offsets, slots_end = plan_slots(sizes)
        self._chunk_job, chunk_off = plan_chunks(sizes, self.chunk_bytes)
        self.nchunks = len(self._chunk_job)
        self._sum_off = slots_end
        self._bad_off = slots_end + 8 * self.nchunks
        total = -(-(self._bad_off + 4 * self.nchunks) // SLOT_ALIGN) * SLOT_ALIGN
        self.state_bytes = sum(sizes)
        self.staging = torch.zeros(max(total, SLOT_ALIGN), dtype=torch.uint8, device=dev)
        self._host = torch.zeros(self.staging.numel(), dtype=torch.uint8, pin_memory=True)
        base = self.staging.data_ptr()
        assert base % SLOT_ALIGN == 0
        rows = []
        for t, size, off in zip(self._blocks, sizes, offsets):   # spv_copy_job: src, dst, bytes, (kind, reserved)
            rows += [t.data_ptr(), base + off, size, 1 if t.dtype == torch.float32 else 0]
        self._jobs = torch.tensor(rows, dtype=torch.int64).to(dev)
        self._chunk_job_dev = torch.tensor(self._chunk_job, dtype=torch.int32).to(dev)
        self._chunk_off_dev = torch.tensor(chunk_off, dtype=torch.int64).to(dev)
        self.metas = [dict(name=n, dtype=_dtype_name(t.dtype), shape=tuple(t.shape), bytes=int(s), offset=int(o))
                      for (n, t), s, o in zip(named_blocks, sizes, offsets)]
        self._slots_end = slots_end
        self._taken = torch.cuda.Event()
        self._copied = torch.cuda.Event()
        self._side = torch.cuda.Stream(device=dev)
        self._writer = _Writer()
        self._call = _native.call
        self.closed = False

    def launch(self, stream=None):
        """the ONE launch: every block into its slot, the partials behind the slots (captured as it is: nothing is allocated)"""
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        base = self.staging.data_ptr()
        self._call("spv_snapshot_multi", self._jobs.data_ptr(), self._chunk_job_dev.data_ptr(), self._chunk_off_dev.data_ptr(),
                   self.nchunks, self.chunk_bytes, base + self._sum_off, base + self._bad_off, st)

    def _collect(self, result, wait_ms):
        if result is not None and self.report is not None:
            kind = next(iter(result))
            if kind == "Checkpoint":
                result[kind]["wait_ms"] = wait_ms
            self.report(result)

    def take(self, host_part, epoch):
        """a checkpoint of the blocks as the stream's work so far leaves them; returns without waiting for the device.  A previous
        write still in flight is waited for first (timed: the finished record's "wait_ms")."""
        if self.closed:
            raise RuntimeError("this StateSnapshot was closed")
        self._collect(*self._writer.wait())   # the staging and host buffers are free again
        t0 = time.perf_counter()
        self.launch()
        cur = torch.cuda.current_stream()
        self._taken.record(cur)
        self._side.wait_event(self._taken)
        with torch.cuda.stream(self._side):
            self._host.copy_(self.staging, non_blocking=True)
            self._copied.record(self._side)
        take_ms = (time.perf_counter() - t0) * 1e3
        self._writer.submit(lambda: self._write(host_part, epoch, take_ms))

    def _write(self, host_part, epoch, take_ms):
        self._copied.synchronize()
        t0 = time.perf_counter()
        host = self._host.numpy()
        sums = host[self._sum_off:self._sum_off + 8 * self.nchunks].view("<u8")
        bad = host[self._bad_off:self._bad_off + 4 * self.nchunks].view("<i4")
        sums, bad = fold_partials(self._chunk_job, sums.tolist(), bad.tolist(), len(self.metas))
        rec = commit(self.path, host_part, self.metas, memoryview(host[:self._slots_end]), sums, bad, self.gated, epoch)
        if "Checkpoint" in rec:
            rec["Checkpoint"].update(take_ms=take_ms, wait_ms=0.0, write_ms=(time.perf_counter() - t0) * 1e3)
        return rec

    def close(self):
        """joins the writer: a pending write is finished (and reported) first"""
        if self.closed:
            return
        self.closed = True
        self._collect(*self._writer.close())
