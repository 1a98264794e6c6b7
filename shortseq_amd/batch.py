"""Batch API on the GPU — torch CUDA tensors in, torch CUDA tensors out, one HIP kernel per call.

This is the data-parallel hot path behind the C ABI in
include/shortseq_amd.h.  PyTorch only provides device memory, streams and the caching allocator;
every byte of encode / decode / hamming / counting is done by the HIP kernels in csrc/.

Packed words are returned as int64 tensors holding the raw 64-bit patterns (view them as uint64 on
the host: ``t.cpu().numpy().view(np.uint64)``).  Layout: read i -> words[i, 0:wpr], nt j in word
j // 32 at bits 2*(j % 32), codes A=0 C=1 T=2 G=3 (README.md:101-112).

Errors: a batch containing a read the reference would reject raises the reference's exception for
the FIRST such read in input order (the one ShortSeqCounter's loop, counter.pyx:22-29, would hit):
``Exception("Unsupported base character: X")`` / ``UnicodeDecodeError`` / ``Exception("Sequences
longer than 1024 bases are not supported.")``, with ``.read_index`` set.  The kernels only flag the
read; its exact message comes from re-scanning that one read with the host codec.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ._native import SS_EFULL, NativeError, SsErr, check, lib

MAX_NT = 1024
_NO_BAD = -1  # UINT64_MAX viewed as int64

__all__ = ["words_for", "wpr_for", "encode", "encode_var", "decode", "decode_var", "hamming_ref",
           "hamming_pair", "encode_hamming_ref", "synth_reads", "synth_pool_reads", "synth_zipf_reads", "zipf_cdf",
           "GpuCounter",
           "raise_read_error", "first_bad_buffer", "fastq_index", "gather_rows", "trim_adapter", "host_trim_adapter",
           "trim_quality", "host_trim_quality", "slice_fixed",
           "slice_var", "hamming_all_pairs", "hamming_nearest", "cluster_pairs", "umi_cluster",
           "GROUPED_ROW_TILE", "hamming_all_pairs_grouped", "umi_cluster_grouped", "HostStager", "host_stager", "encode_host", "decode_host"]


def words_for(L: int) -> int:
    """ceil(L / 32): util.pyx:30-33."""
    return (L + 31) // 32


def wpr_for(L: int) -> int:
    """Words per read in batch layouts: 1 for L <= 32 (ShortSeq64 keeps one word even for L = 0)."""
    return max(1, words_for(L))


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _require_cuda(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_first_bad_cache: dict = {}


def first_bad_buffer(dev: torch.device) -> torch.Tensor:
    """Per-device 1-word scratch the kernels atomicMin the first invalid read index into."""
    key = (dev.type, dev.index)
    t = _first_bad_cache.get(key)
    if t is None:
        t = torch.empty(1, dtype=torch.int64, device=dev)
        _first_bad_cache[key] = t
    return t


def raise_read_error(read: bytes, read_index: int) -> None:
    """Raise exactly what shortseq.pack(read) raises in the reference (SURVEY §8 error contract)."""
    if len(read) > MAX_NT:
        e = Exception(f"Sequences longer than {MAX_NT} bases are not supported.")  # short_seq.pyx:74
        e.read_index = read_index
        raise e
    buf = np.frombuffer(read, dtype=np.uint8) if read else np.zeros(1, np.uint8)
    words = np.zeros(32, dtype=np.uint64)
    err = SsErr()
    rc = lib().ss_host_encode(buf.ctypes.data, len(read), words.ctypes.data, C.byref(err))
    if rc == 0:
        raise AssertionError(f"read {read_index} was flagged by the GPU but encodes on the host")
    bad = read[err.byte_offset: err.byte_offset + err.nbytes]
    # short_seq_64.pyx:105 / util.pyx:115,137 — PyUnicode_DecodeASCII of the byte(s); a non-ASCII
    # byte makes that decode itself raise UnicodeDecodeError, as in the reference.
    e = Exception(f"Unsupported base character: {bad.decode('ascii')}")
    e.read_index = read_index
    raise e


def _check_first_bad(fb: torch.Tensor, fetch_read) -> None:
    v = int(fb.item())
    if v != _NO_BAD:
        raise_read_error(fetch_read(v), v)


def _as_rows(ascii: torch.Tensor, L: Optional[int], stride: Optional[int]):
    _require_cuda(ascii, "ascii")
    if ascii.dtype != torch.uint8:
        raise TypeError("ascii must be a uint8 tensor")
    if ascii.dim() == 2:
        n, width = ascii.shape
        L = width if L is None else L
        stride = width if stride is None else stride
        if stride != width:
            raise ValueError("for a 2-D ascii tensor the stride is its row width")
    else:
        if L is None:
            raise ValueError("L is required for a flat ascii tensor")
        stride = L if stride is None else stride
        n = ascii.numel() // stride if stride else 0
    if not (1 <= L <= MAX_NT):
        if L > MAX_NT:
            raise Exception(f"Sequences longer than {MAX_NT} bases are not supported.")
        raise ValueError("L must be >= 1 (empty reads are the empty singleton, no kernel needed)")
    if stride < L:
        raise ValueError("stride < L")
    return n, L, stride


def _fetch_row(ascii: torch.Tensor, stride: int, L: int):
    flat = ascii.reshape(-1)
    return lambda i: bytes(flat[i * stride: i * stride + L].cpu().numpy())


def encode(ascii: torch.Tensor, L: Optional[int] = None, *, stride: Optional[int] = None,
           wpr: Optional[int] = None, out: Optional[torch.Tensor] = None,
           check_errors: bool = True) -> torch.Tensor:
    """Encode a fixed-length batch (one ss_encode_fixed launch).  ascii: uint8 [n, L] or flat."""
    n, L, stride = _as_rows(ascii, L, stride)
    wpr = wpr_for(L) if wpr is None else wpr
    dev = ascii.device
    if out is None:
        out = torch.empty((n, wpr), dtype=torch.int64, device=dev)
    fb = first_bad_buffer(dev)
    check(lib().ss_encode_fixed(ascii.data_ptr(), n, L, stride, out.data_ptr(), wpr, fb.data_ptr(),
                                _stream(dev)), "ss_encode_fixed")
    if check_errors:
        _check_first_bad(fb, _fetch_row(ascii, stride, L))
    return out


def encode_var(blob: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, *,
               wpr: Optional[int] = None, out: Optional[torch.Tensor] = None,
               check_errors: bool = True) -> torch.Tensor:
    """Encode a ragged batch: read i = blob[offsets[i] : offsets[i] + lens[i]] (0..1024 nt)."""
    for t, nm in ((blob, "blob"), (offsets, "offsets"), (lens, "lens")):
        _require_cuda(t, nm)
    if offsets.dtype != torch.int64 or lens.dtype != torch.int32 or blob.dtype != torch.uint8:
        raise TypeError("blob uint8, offsets int64, lens int32 expected")
    n = lens.numel()
    if wpr is None:
        wpr = wpr_for(min(int(lens.max().item()), MAX_NT)) if n else 1
    dev = blob.device
    if out is None:
        out = torch.empty((n, wpr), dtype=torch.int64, device=dev)
    fb = first_bad_buffer(dev)
    check(lib().ss_encode_var(blob.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n, out.data_ptr(),
                              wpr, fb.data_ptr(), _stream(dev)), "ss_encode_var")
    if check_errors:
        def fetch(i):
            o, ln = int(offsets[i].item()), int(lens[i].item())
            return bytes(blob[o:o + ln].cpu().numpy())
        _check_first_bad(fb, fetch)
    return out


def decode(words: torch.Tensor, L: int, *, wpr: Optional[int] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed words [n, wpr] -> ASCII uint8 [n, L] (one ss_decode_fixed launch)."""
    _require_cuda(words, "words")
    wpr = words.shape[1] if words.dim() == 2 else (wpr_for(L) if wpr is None else wpr)
    n = words.numel() // wpr
    dev = words.device
    if out is None:
        out = torch.empty((n, L), dtype=torch.uint8, device=dev)
    check(lib().ss_decode_fixed(words.data_ptr(), n, L, wpr, out.data_ptr(), L, _stream(dev)),
          "ss_decode_fixed")
    return out


def decode_var(words: torch.Tensor, lens: torch.Tensor, offsets: torch.Tensor,
               out_bytes: Optional[int] = None) -> torch.Tensor:
    """Ragged decode into one blob; read i lands at blob[offsets[i] : offsets[i] + lens[i]]."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    dev = words.device
    total = out_bytes if out_bytes is not None else (
        int((offsets[-1] + lens[-1]).item()) if n else 0)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    check(lib().ss_decode_var(words.data_ptr(), lens.data_ptr(), n, wpr, out.data_ptr(),
                              offsets.data_ptr(), _stream(dev)), "ss_decode_var")
    return out[:total]


def hamming_ref(words: torch.Tensor, L: int, ref: torch.Tensor) -> torch.Tensor:
    """Per-read __xor__ distance to one packed reference read -> int32 [n]."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    out = torch.empty(n, dtype=torch.int32, device=words.device)
    ref = ref.to(words.device).contiguous()
    check(lib().ss_hamming_ref(words.data_ptr(), n, L, wpr, ref.data_ptr(), out.data_ptr(),
                               _stream(words.device)), "ss_hamming_ref")
    return out


def hamming_pair(a: torch.Tensor, b: torch.Tensor, L: int) -> torch.Tensor:
    """Element-wise a[i] ^ b[i] (ShortSeq.__xor__) -> int32 [n]."""
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape")
    n, wpr = a.shape
    out = torch.empty(n, dtype=torch.int32, device=a.device)
    check(lib().ss_hamming_pair(a.data_ptr(), b.data_ptr(), n, L, wpr, out.data_ptr(), _stream(a.device)),
          "ss_hamming_pair")
    return out


def encode_hamming_ref(ascii: torch.Tensor, L: Optional[int], ref_words: torch.Tensor, *,
                       store_words: bool = True, wpr: Optional[int] = None,
                       check_errors: bool = True):
    """Fused encode + hamming vs one packed reference: returns (words or None, distances int32)."""
    n, L, stride = _as_rows(ascii, L, None if ascii.dim() == 2 else L)
    wpr = wpr_for(L) if wpr is None else wpr
    dev = ascii.device
    words = torch.empty((n, wpr), dtype=torch.int64, device=dev) if store_words else None
    dist = torch.empty(n, dtype=torch.int32, device=dev)
    ref = ref_words.to(dev).contiguous()
    if ref.numel() < wpr:
        ref = torch.cat([ref.reshape(-1), torch.zeros(wpr - ref.numel(), dtype=torch.int64, device=dev)])
    fb = first_bad_buffer(dev)
    check(lib().ss_encode_hamming_ref(ascii.data_ptr(), n, L, stride, _ptr(words), wpr, ref.data_ptr(),
                                      dist.data_ptr(), fb.data_ptr(), _stream(dev)),
          "ss_encode_hamming_ref")
    if check_errors:
        _check_first_bad(fb, _fetch_row(ascii, stride, L))
    return words, dist


def _host_rows(ascii, L: Optional[int], stride: Optional[int]):
    """numpy uint8 [n, >=L] (rows may be padded: stride = row pitch) or flat bytes-like + L."""
    a = np.frombuffer(ascii, dtype=np.uint8) if isinstance(ascii, (bytes, bytearray, memoryview)) else ascii
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise TypeError("host reads must be a uint8 numpy array or a bytes-like object")
    if a.ndim == 2:
        if a.strides[1] != 1 or (a.shape[0] > 1 and a.strides[0] < a.shape[1]):
            raise ValueError("rows must be contiguous bytes")
        L = a.shape[1] if L is None else L
        stride = a.strides[0] if a.shape[0] > 1 else a.shape[1]
        n = a.shape[0]
    else:
        if L is None:
            raise ValueError("L is required for a flat host buffer")
        a = np.ascontiguousarray(a).reshape(-1)
        stride = L if stride is None else stride
        n = a.size // stride if stride else 0
    if not (1 <= L <= MAX_NT):
        if L > MAX_NT:
            raise Exception(f"Sequences longer than {MAX_NT} bases are not supported.")
        raise ValueError("L must be >= 1")
    if stride < L:
        raise ValueError("stride < L")
    return a, n, L, stride


class HostStager:
    """Host-resident batches through the GPU (ss_stager_*, csrc/ss_stage.hip): numpy in, numpy out.

    A batch in host memory is streamed through a ring of pinned + device chunk slots on three HIP
    streams (H2D / kernel / D2H overlapped across neighbouring chunks).  Pageable arrays are staged
    by `copy_threads` memcpy threads; pinned arrays (torch .pin_memory().numpy()) are DMA'd
    directly.  This is the PCIe-inclusive path for data that lives on the host; for data already
    in HBM use encode()/decode() on tensors."""

    def __init__(self, device=None, chunk_bytes: int = 64 << 20, nslots: int = 3,
                 copy_threads: Optional[int] = None):
        import os
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        if copy_threads is None:
            # 12 threads pinned to the GPU's NUMA node: 20.0 ms for 32M x 32-nt reads against 21.4
            # with 8 and 20.6 with 16, the H2D copies at ~19 ms the floor (profiles/r6/probe_stage_split.log)
            copy_threads = int(os.environ.get("SHORTSEQ_STAGE_THREADS", min(12, os.cpu_count() or 1)))
        h = C.c_void_p()
        check(lib().ss_stager_create(self.device.index or 0, chunk_bytes, nslots, copy_threads, C.byref(h)),
              "ss_stager_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ss_stager_destroy(self._h)
            self._h = None

    STAGES = ("copy_in_host", "copy_out_host", "h2d_dev", "kernel_dev", "d2h_dev", "wait_host")

    def set_timing(self, on: bool = True) -> None:
        """Record the per-chunk stage split (ss_stager_set_timing)."""
        check(lib().ss_stager_set_timing(self._h, int(bool(on))), "ss_stager_set_timing")

    def stats(self) -> dict:
        """Mean ms per timed call of each stage since the last stats() (device stages are sums over
        chunks, which overlap), and the placement: copy threads, affinity CPUs, the GPU's NUMA node,
        CPUs the copy threads are pinned to (ss_stager_stats)."""
        ms = (C.c_double * 6)()
        info = (C.c_int32 * 4)()
        check(lib().ss_stager_stats(self._h, ms, info), "ss_stager_stats")
        out = {k: float(v) for k, v in zip(self.STAGES, ms)}
        out.update(copy_threads=int(info[0]), affinity_cpus=int(info[1]), gpu_numa_node=int(info[2]),
                   pinned_cpus=int(info[3]))
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass

    @staticmethod
    def _raise_first_bad(fb: int, a: np.ndarray, stride: int, L: int) -> None:
        if fb != (1 << 64) - 1:
            row = a[fb, :L] if a.ndim == 2 else a[fb * stride: fb * stride + L]
            raise_read_error(bytes(row), fb)

    def encode(self, ascii, L: Optional[int] = None, *, stride: Optional[int] = None, wpr: Optional[int] = None,
               out: Optional[np.ndarray] = None, check_errors: bool = True) -> np.ndarray:
        """-> packed words uint64 [n, wpr] in host memory (ss_encode_host)."""
        a, n, L, stride = _host_rows(ascii, L, stride)
        wpr = wpr_for(L) if wpr is None else wpr
        if out is None:
            out = np.empty((n, wpr), dtype=np.uint64)
        fb = C.c_uint64()
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_encode_host(self._h, a.ctypes.data, n, L, stride, out.ctypes.data, wpr, C.byref(fb)),
              "ss_encode_host")
        if check_errors:
            self._raise_first_bad(fb.value, a, stride, L)
        return out

    def encode_hamming_ref(self, ascii, L: Optional[int], ref_words, *, check_errors: bool = True):
        """-> (words uint64 [n, wpr], distances uint32 [n]) vs one packed reference read."""
        a, n, L, stride = _host_rows(ascii, L, None)
        wpr = wpr_for(L)
        ref = torch.zeros(wpr, dtype=torch.int64, device=self.device)
        r = torch.as_tensor(np.asarray(ref_words, dtype=np.uint64).view(np.int64)).reshape(-1)[:wpr]
        ref[:r.numel()] = r.to(self.device)
        torch.cuda.current_stream(self.device).synchronize()
        words = np.empty((n, wpr), dtype=np.uint64)
        dist = np.empty(n, dtype=np.uint32)
        fb = C.c_uint64()
        check(lib().ss_encode_hamming_ref_host(self._h, a.ctypes.data, n, L, stride, words.ctypes.data, wpr,
                                               ref.data_ptr(), dist.ctypes.data, C.byref(fb)),
              "ss_encode_hamming_ref_host")
        if check_errors:
            self._raise_first_bad(fb.value, a, stride, L)
        return words, dist

    def decode(self, words: np.ndarray, L: int, *, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Packed words uint64 [n, wpr] (host) -> ASCII uint8 [n, L] (host) (ss_decode_host)."""
        w = np.ascontiguousarray(words)
        if w.dtype not in (np.uint64, np.int64):
            raise TypeError("words must be uint64 / int64")
        if w.ndim == 1:
            w = w.reshape(-1, wpr_for(L))
        n, wpr = w.shape
        if out is None:
            out = np.empty((n, L), dtype=np.uint8)
        check(lib().ss_decode_host(self._h, w.ctypes.data, n, L, wpr, out.ctypes.data, out.strides[0] if n else L),
              "ss_decode_host")
        return out


_stagers: dict = {}


def host_stager(device=None) -> HostStager:
    """The process's default HostStager for a device (created on first use)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    st = _stagers.get(dev.index)
    if st is None:
        st = _stagers[dev.index] = HostStager(dev)
    return st


def encode_host(ascii, L: Optional[int] = None, **kw) -> np.ndarray:
    """Host array of reads -> host array of packed words, streamed through the GPU."""
    return host_stager(kw.pop("device", None)).encode(ascii, L, **kw)


def decode_host(words: np.ndarray, L: int, **kw) -> np.ndarray:
    return host_stager(kw.pop("device", None)).decode(words, L, **kw)


def synth_reads(n: int, L: int, seed: int, *, i0: int = 0, device=None, stride: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device-side synthetic reads (SURVEY §8(d) generator, bit-identical to the oracle's)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    stride = L if stride is None else stride
    if out is None:
        out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    check(lib().ss_synth_reads(out.data_ptr(), seed, i0, n, L, stride, _stream(dev)), "ss_synth_reads")
    return out


def synth_pool_reads(n: int, L: int, seed: int, pool_seed: int, U: int, *, i0: int = 0, device=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((n, L), dtype=torch.uint8, device=dev)
    check(lib().ss_synth_pool_reads(out.data_ptr(), seed, pool_seed, U, i0, n, L, L, _stream(dev)),
          "ss_synth_pool_reads")
    return out


def zipf_cdf(U: int, s: float = 1.1) -> np.ndarray:
    """Zipf(s) CDF over pool ranks 0..U-1 scaled to 2^63 (uint64 [U]; the last entry is 2^63), the
    table ss_synth_zipf_reads draws from (include/shortseq_amd.h).  Rank k has weight (k+1)^-s."""
    w = np.arange(1, U + 1, dtype=np.float64) ** (-float(s))
    c = np.cumsum(w)
    c /= c[-1]
    cdf = np.floor(c * 2.0 ** 63).astype(np.uint64)
    cdf[-1] = np.uint64(1 << 63)
    return cdf


def synth_zipf_reads(n: int, L: int, seed: int, pool_seed: int, cdf, *, i0: int = 0, device=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reads drawn from a Zipf-distributed pool (SURVEY §8(d) C5 skew): read i = pool item
    rank(i) of the ss_synth_zipf_reads rule; `cdf` = zipf_cdf(U, s) (numpy) or its device copy."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if isinstance(cdf, np.ndarray):
        cdf = torch.from_numpy(cdf.view(np.int64)).to(dev)
    if out is None:
        out = torch.empty((n, L), dtype=torch.uint8, device=dev)
    check(lib().ss_synth_zipf_reads(out.data_ptr(), seed, pool_seed, cdf.data_ptr(), cdf.numel(), i0, n, L, L,
                                    _stream(dev)), "ss_synth_zipf_reads")
    return out


def synth_ragged_pool_reads(n: int, seed: int, pool_seed: int, U: int, Lmin: int, Lmax: int, *, i0: int = 0,
                            device=None):
    """Device-side ragged reads drawn from a pool of U items of lengths Lmin..Lmax (the
    ss_synth_ragged_* rule, include/shortseq_amd.h): returns (blob u8 [total + 16], offsets i64 [n],
    lens i32 [n]) with the reads back to back."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    s = _stream(dev)
    check(lib().ss_synth_ragged_lens(lens.data_ptr(), seed, pool_seed, U, i0, n, Lmin, Lmax, s), "ss_synth_ragged_lens")
    offs = torch.cumsum(lens, 0, dtype=torch.int64) - lens.to(torch.int64)   # layout only (exclusive prefix)
    total = int(offs[-1].item() + lens[-1].item()) if n else 0
    blob = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    check(lib().ss_synth_ragged_reads(blob.data_ptr(), offs.data_ptr(), seed, pool_seed, U, i0, n, Lmin, Lmax, s),
          "ss_synth_ragged_reads")
    return blob, offs, lens


def _adapter_bytes(adapter, min_overlap: int, err_div: int) -> bytes:
    """The adapter as bytes (str: its ASCII), with the argument checks of the C ABI raised as ValueError."""
    if isinstance(adapter, str):
        adapter = adapter.encode("ascii")
    adapter = bytes(adapter)
    if not 1 <= len(adapter) <= 64:
        raise ValueError("adapter of 1 .. 64 bytes expected")
    if min_overlap < 1:
        raise ValueError("min_overlap >= 1 expected")
    if err_div < 0:
        raise ValueError("err_div >= 0 expected")
    return adapter


def trim_adapter(blob: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, adapter, *, min_overlap: int = 3,
                 err_div: int = 10, out: Optional[torch.Tensor] = None, stats: bool = False, _reads_per_launch: int = 0):
    """3' adapter trim of a ragged batch (one ss_trim_adapter3 launch): the new length of read i =
    blob[offsets[i] : offsets[i] + lens[i]] is the least position p at which `adapter` (bytes or str, 1..64
    bytes, 'N' = wildcard) matches with overlap ov = min(len(adapter), lens[i] - p) >= min_overlap and at
    most ov // err_div mismatches (err_div 0: none), or lens[i].  Leftmost match, no indels; the read's
    bytes are compared as they are.  Reads longer than 1024 keep their length.  No read is moved:
    (offsets, new lens) feed encode_var / DeviceIngest.count as they are.  `out` may be `lens` itself.
    stats=True also returns an int64 [2] tensor {reads shortened, bytes removed}."""
    for t, nm in ((blob, "blob"), (offsets, "offsets"), (lens, "lens")):
        _require_cuda(t, nm)
    if offsets.dtype != torch.int64 or lens.dtype not in (torch.int32, torch.uint32) or blob.dtype != torch.uint8:
        raise TypeError("blob uint8, offsets int64, lens int32 expected")
    a = _adapter_bytes(adapter, min_overlap, err_div)
    n = lens.numel()
    if offsets.numel() != n:
        raise ValueError("offsets and lens differ in length")
    dev = blob.device
    if out is None:
        out = torch.empty_like(lens)
    else:
        _require_cuda(out, "out")
        if out.dtype != lens.dtype or out.numel() != n:
            raise ValueError("out must match lens")
    st = torch.empty(2, dtype=torch.int64, device=dev) if stats else None
    abuf = (C.c_uint8 * len(a)).from_buffer_copy(a)
    check(lib().ss_trim_adapter3_ex(blob.data_ptr(), blob.numel(), offsets.data_ptr(), lens.data_ptr(), n, abuf, len(a),
                                    min_overlap, err_div, out.data_ptr(), _ptr(st), _reads_per_launch, _stream(dev)),
          "ss_trim_adapter3")
    return (out, st) if stats else out


def host_trim_adapter(blob, offsets, lens, adapter, *, min_overlap: int = 3, err_div: int = 10, out=None,
                      stats: bool = False):
    """trim_adapter on numpy arrays (ss_host_trim_adapter3, plain C++): blob uint8, offsets uint64 / int64,
    lens uint32 / int32.  Also checks that every read of at most 1024 bytes lies inside the blob."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets)
    lens = np.ascontiguousarray(lens)
    if offsets.dtype not in (np.uint64, np.int64) or lens.dtype not in (np.uint32, np.int32):
        raise TypeError("blob uint8, offsets uint64, lens uint32 expected")
    a = _adapter_bytes(adapter, min_overlap, err_div)
    n = lens.size
    if offsets.size != n:
        raise ValueError("offsets and lens differ in length")
    if out is None:
        out = np.empty_like(lens)
    elif out.dtype != lens.dtype or out.size != n or not out.flags.c_contiguous:
        raise ValueError("out must match lens")
    st = np.zeros(2, dtype=np.uint64) if stats else None
    abuf = (C.c_uint8 * len(a)).from_buffer_copy(a)
    check(lib().ss_host_trim_adapter3(blob.ctypes.data, blob.size, offsets.ctypes.data, lens.ctypes.data, n, abuf, len(a),
                                      min_overlap, err_div, out.ctypes.data, st.ctypes.data if stats else None),
          "ss_host_trim_adapter3")
    return (out, st) if stats else out


def _quality_args(cutoff: int, base: int) -> None:
    """The argument checks of ss_trim_quality3 raised as ValueError."""
    if not 1 <= cutoff <= 93:
        raise ValueError("quality cutoff in 1 .. 93 expected")
    if base not in (33, 64):
        raise ValueError("quality base of 33 or 64 expected")


def trim_quality(blob: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, cutoff: int, *, base: int = 33,
                 qual: Optional[torch.Tensor] = None, qoffsets: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, stats: bool = False, _reads_per_launch: int = 0):
    """3' quality trim of a ragged batch (one ss_trim_quality3 launch): BWA's running sum from the read's
    right end, s += cutoff - (q - base) per quality byte, stopped where s < 0; the new length is the
    rightmost position of the greatest s > 0, or lens[i] (include/shortseq_amd.h, "3' quality trim").
    With `qual` and `qoffsets` read i's qualities are the lens[i] bytes at qual[qoffsets[i]:]; without
    them `blob` is FASTQ text, (offsets, lens) its fastq_index, and each read's quality line is found
    behind its '+' line (a read without a quality line of lens[i] bytes keeps its length).  Reads longer
    than 1024 keep their length.  No read is moved: (offsets, new lens) feed trim_adapter, encode_var and
    DeviceIngest.count as they are.  `out` may be `lens` itself.  stats=True also returns an int64 [3]
    tensor {reads shortened, bytes removed, reads without a usable quality line}."""
    for t, nm in ((blob, "blob"), (offsets, "offsets"), (lens, "lens")):
        _require_cuda(t, nm)
    if offsets.dtype != torch.int64 or lens.dtype not in (torch.int32, torch.uint32) or blob.dtype != torch.uint8:
        raise TypeError("blob uint8, offsets int64, lens int32 expected")
    _quality_args(cutoff, base)
    n = lens.numel()
    if offsets.numel() != n:
        raise ValueError("offsets and lens differ in length")
    if (qual is None) != (qoffsets is None):
        raise ValueError("qual and qoffsets go together")
    if qual is not None:
        _require_cuda(qual, "qual")
        _require_cuda(qoffsets, "qoffsets")
        if qual.dtype != torch.uint8 or qoffsets.dtype != torch.int64 or qoffsets.numel() != n:
            raise TypeError("qual uint8, qoffsets int64 of the reads' count expected")
    dev = blob.device
    if out is None:
        out = torch.empty_like(lens)
    else:
        _require_cuda(out, "out")
        if out.dtype != lens.dtype or out.numel() != n:
            raise ValueError("out must match lens")
    st = torch.empty(3, dtype=torch.int64, device=dev) if stats else None
    check(lib().ss_trim_quality3_ex(blob.data_ptr(), blob.numel(), offsets.data_ptr(), lens.data_ptr(), n, _ptr(qual),
                                    _ptr(qoffsets), cutoff, base, out.data_ptr(), _ptr(st), _reads_per_launch,
                                    _stream(dev)), "ss_trim_quality3")
    return (out, st) if stats else out


def host_trim_quality(blob, offsets, lens, cutoff: int, *, base: int = 33, qual=None, qoffsets=None, out=None,
                      stats: bool = False):
    """trim_quality on numpy arrays (ss_host_trim_quality3, plain C++): blob and qual uint8, offsets and
    qoffsets uint64 / int64, lens uint32 / int32.  Also checks that every read of at most 1024 bytes lies
    inside the blob and, with `qual`, its quality run inside `qual`."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets)
    lens = np.ascontiguousarray(lens)
    if offsets.dtype not in (np.uint64, np.int64) or lens.dtype not in (np.uint32, np.int32):
        raise TypeError("blob uint8, offsets uint64, lens uint32 expected")
    _quality_args(cutoff, base)
    n = lens.size
    if offsets.size != n:
        raise ValueError("offsets and lens differ in length")
    if (qual is None) != (qoffsets is None):
        raise ValueError("qual and qoffsets go together")
    if qual is not None:
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        qoffsets = np.ascontiguousarray(qoffsets)
        if qoffsets.dtype not in (np.uint64, np.int64) or qoffsets.size != n:
            raise TypeError("qoffsets uint64 of the reads' count expected")
    if out is None:
        out = np.empty_like(lens)
    elif out.dtype != lens.dtype or out.size != n or not out.flags.c_contiguous:
        raise ValueError("out must match lens")
    st = np.zeros(3, dtype=np.uint64) if stats else None
    check(lib().ss_host_trim_quality3(blob.ctypes.data, blob.size, offsets.ctypes.data, lens.ctypes.data, n,
                                      None if qual is None else qual.ctypes.data, 0 if qual is None else qual.size,
                                      None if qual is None else qoffsets.ctypes.data, cutoff, base, out.ctypes.data,
                                      st.ctypes.data if stats else None), "ss_host_trim_quality3")
    return (out, st) if stats else out


class DeviceIngest:
    """The drop-in counter's engine (ss_ingest_*) fed from device memory: count(blob, offsets, lens)
    any number of times (global read indices continue), then results() -> (lens u32, counts u64,
    words u64) numpy arrays in first-occurrence order (the ShortSeqCounter dict order: row k has
    ceil(lens[k] / 32) words, one for lengths 0..32).  A rejected read raises like ShortSeqCounter."""

    def __init__(self, device=None, exact: bool = False, *, compact=True, _sizing: Optional[int] = None,
                 adapter=None, min_overlap: int = 3, err_div: int = 10):
        """compact: the rows cross PCIe with u16 lengths and u32 counts (u64 when a count needs it):
        results() then returns those dtypes (ss_ingest_set_results_format).
        adapter (bytes or str): every batch is 3'-trimmed on the device first (the rule of trim_adapter,
        ss_ingest_set_adapter); the caller's lens tensor is not written."""
        a = None if adapter is None else _adapter_bytes(adapter, min_overlap, err_div)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        h = C.c_void_p()
        check(lib().ss_ingest_create(dev.index or 0, C.byref(h)), "ss_ingest_create")
        self._h = h
        self.compact = int(compact)      # (2: compact with u64 counts, a test hook)
        check(lib().ss_ingest_set_results_format(h, self.compact), "ss_ingest_set_results_format")
        self._exact = exact
        self._sizing = int(exact) if _sizing is None else _sizing   # 2: test hook, undersized class tables
        self._fresh = True
        check(lib().ss_ingest_set_exact(h, self._sizing), "ss_ingest_set_exact")
        if a is not None:
            check(lib().ss_ingest_set_adapter(h, (C.c_uint8 * len(a)).from_buffer_copy(a), len(a), min_overlap, err_div),
                  "ss_ingest_set_adapter")

    def count(self, blob: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor) -> None:
        for t, name in ((blob, "blob"), (offsets, "offsets"), (lens, "lens")):
            _require_cuda(t, name)
        if offsets.dtype != torch.int64 or lens.dtype not in (torch.int32, torch.uint32) or blob.dtype != torch.uint8:
            raise TypeError("blob u8, offsets int64, lens int32")
        torch.cuda.current_stream(self.device).synchronize()   # the engine runs on its own stream
        args = (self._h, blob.data_ptr(), blob.numel(), offsets.data_ptr(), lens.data_ptr(), lens.numel())
        rc = lib().ss_ingest_add_device(*args)
        self.retried = False
        if rc == SS_EFULL and self._fresh and not self._exact:
            # a length class's table, sized by its distinct-key sketch, ran full: the first batch of the
            # count is counted again with tables sized by their rows (later batches cannot be redone)
            check(lib().ss_ingest_reset(self._h), "ss_ingest_reset")
            check(lib().ss_ingest_set_exact(self._h, 1), "ss_ingest_set_exact")
            rc = lib().ss_ingest_add_device(*args)
            check(lib().ss_ingest_set_exact(self._h, self._sizing), "ss_ingest_set_exact")
            self.retried = True
        if rc == SS_EFULL and not self._fresh:
            raise NativeError("ss_ingest_add_device: a length class's table, sized by its distinct-key "
                                  "sketch, ran full on a later batch; the counts so far are void -- reset() "
                                  "and count every batch again with DeviceIngest(exact=True)")
        check(rc, "ss_ingest_add_device")
        self._fresh = False
        idx, kind, ln = C.c_uint64(), C.c_int(), C.c_uint64()
        check(lib().ss_ingest_error(self._h, C.byref(idx), C.byref(kind), None, 0, C.byref(ln)), "ss_ingest_error")
        if idx.value != (1 << 64) - 1:
            if kind.value == 2:
                raise Exception("Sequences longer than 1024 bases are not supported.")
            buf = (C.c_uint8 * max(1, ln.value))()
            check(lib().ss_ingest_error(self._h, C.byref(idx), C.byref(kind), buf, ln.value, C.byref(ln)),
                  "ss_ingest_error")
            raise_read_error(bytes(buf)[:ln.value], idx.value)

    def results(self, copy: bool = True):
        """(lens, counts, words u64) of the count so far, first-occurrence order: lens u32 and counts
        u64, or with compact=True lens u16 and counts u32 (u64 when a count needs it).  copy=False
        returns views of the engine's pinned result buffers, valid until the next count / reset /
        close (no host-side copy of the rows)."""
        K, NW = C.c_uint64(), C.c_uint64()
        check(lib().ss_ingest_finish(self._h, C.byref(K), C.byref(NW)), "ss_ingest_finish")
        pl, pc, pw = C.c_void_p(), C.c_void_p(), C.c_void_p()
        k, nw = K.value, NW.value
        if self.compact:
            cb = C.c_uint32()
            check(lib().ss_ingest_results_compact(self._h, C.byref(pl), C.byref(pc), C.byref(cb), C.byref(pw)),
                  "ss_ingest_results_compact")
            lt, ct = C.c_uint16, (C.c_uint32 if cb.value == 4 else C.c_uint64)
        else:
            check(lib().ss_ingest_results(self._h, C.byref(pl), C.byref(pc), C.byref(pw)), "ss_ingest_results")
            lt, ct = C.c_uint32, C.c_uint64
        lens = np.ctypeslib.as_array((lt * max(1, k)).from_address(pl.value))[:k] if k else np.zeros(0, lt)
        cnts = np.ctypeslib.as_array((ct * max(1, k)).from_address(pc.value))[:k] if k else np.zeros(0, ct)
        wds = np.ctypeslib.as_array((C.c_uint64 * max(1, nw)).from_address(pw.value))[:nw] if nw else np.zeros(0, np.uint64)
        if copy:
            lens, cnts, wds = lens.copy(), cnts.copy(), wds.copy()
        return lens, cnts, wds

    def set_row_limit(self, rows: int) -> None:
        """Test hook: re-key a length's table once its rows pass `rows` (default 2^32 - 1)."""
        check(lib().ss_ingest_set_row_limit(self._h, int(rows)), "ss_ingest_set_row_limit")

    def set_count_limit(self, reads: int) -> None:
        """Test hook: spill the tables' u32 counts into u64 row counts every `reads` reads (default 2^32 - 2)."""
        check(lib().ss_ingest_set_count_limit(self._h, int(reads)), "ss_ingest_set_count_limit")

    def export(self) -> int:
        """Extract this engine's tables for a device-side reduce (ss_ingest_export); its distinct keys."""
        k = C.c_uint64()
        check(lib().ss_ingest_export(self._h, C.byref(k)), "ss_ingest_export")
        return k.value

    def merge(self, src: "DeviceIngest", base: int) -> None:
        """Fold an exported engine whose reads follow this one's (global read index `base` onward) into
        this engine's tables on its device (ss_ingest_merge: peer copies, counts add, first = min)."""
        check(lib().ss_ingest_merge(self._h, src._h, int(base)), "ss_ingest_merge")

    def reserve_merge(self, srcs) -> None:
        """Size this engine's tables once for the union of the exported engines `srcs` it will merge
        (ss_ingest_reserve_merge): no table growth per merge."""
        arr = (C.c_void_p * max(1, len(srcs)))(*[e._h.value for e in srcs])
        check(lib().ss_ingest_reserve_merge(self._h, arr, len(srcs)), "ss_ingest_reserve_merge")

    def reset(self) -> None:
        check(lib().ss_ingest_reset(self._h), "ss_ingest_reset")
        self._fresh = True

    def close(self) -> None:
        if self._h:
            lib().ss_ingest_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def slice_fixed(words: torch.Tensor, L: int, start: Optional[int] = None, stop: Optional[int] = None,
                *, out: Optional[torch.Tensor] = None):
    """reads[start:stop] for every read of a fixed-length packed batch (Python slice bounds, step 1,
    as ShortSeq.__getitem__; short_seq.pyx:93-238) -> (words [n, max(1, ceil(len/32))], len)."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    st, sp, step = slice(start, stop).indices(L)
    ln = max(0, sp - st)
    if ln == 0:
        st = 0
    ow = wpr_for(ln)
    if out is None:
        out = torch.empty((n, ow), dtype=torch.int64, device=words.device)
    check(lib().ss_slice_fixed(words.data_ptr(), n, L, wpr, st, ln, out.data_ptr(), out.shape[1],
                               _stream(words.device)), "ss_slice_fixed")
    return out, ln


def slice_var(words: torch.Tensor, starts: torch.Tensor, lens: torch.Tensor, *,
              read_lens: Optional[torch.Tensor] = None, out_wpr: Optional[int] = None) -> torch.Tensor:
    """Per-read slices of a packed batch (adapter / UMI trimming): row r = nts [starts[r],
    starts[r] + lens[r]) of read r, clamped to read_lens[r] when given (int32 tensors)."""
    for t, nm in ((words, "words"), (starts, "starts"), (lens, "lens")):
        _require_cuda(t, nm)
    n, wpr = words.shape
    if out_wpr is None:
        out_wpr = wpr
    out = torch.empty((n, out_wpr), dtype=torch.int64, device=words.device)
    check(lib().ss_slice_var(words.data_ptr(), n, wpr, _ptr(read_lens), starts.data_ptr(), lens.data_ptr(),
                             out.data_ptr(), out_wpr, _stream(words.device)), "ss_slice_var")
    return out


ALL_PAIRS_METHODS = {"auto": 0, "tiles": 1, "pigeonhole": 2, "bucketed": 3}


def hamming_all_pairs(words: torch.Tensor, L: int, max_dist: int, *, counts: bool = True,
                      max_pairs: int = 0, method: str = "auto"):
    """Unordered pairs (i < j) of a packed batch within `max_dist` (the reference __xor__ distance)
    -> (neighbour counts int32 [n] or None, pairs int32 [m, 2] or None, total pairs).  Pairs are
    returned sorted; at most max_pairs are kept (0: count only).  method: "tiles" checks every pair,
    "pigeonhole" (L <= 128, max_dist < 16) only pairs sharing one of max_dist + 1 segments,
    "bucketed" the same rule for any L <= 1024 and max_dist <= 31 (past pigeonhole's range the rows
    stay where they are and are read through bucket-ordered indices), "auto" picks
    (ss_hamming_all_pairs_ex); the results are the same."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    dev = words.device
    cnt = torch.empty(n, dtype=torch.int32, device=dev) if counts else None
    pairs = torch.empty((max(1, max_pairs), 2), dtype=torch.int32, device=dev) if max_pairs else None
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib().ss_hamming_all_pairs_ex(words.data_ptr(), n, L, wpr, max_dist, _ptr(cnt), _ptr(pairs), max_pairs,
                                        tot.data_ptr(), ALL_PAIRS_METHODS[method], _stream(dev)),
          "ss_hamming_all_pairs_ex")
    total = int(tot.item())
    if pairs is not None:
        m = min(total, max_pairs)
        p = pairs[:m].to(torch.int64)
        key = p[:, 0] * (1 << 32) + p[:, 1]
        pairs = pairs[:m][torch.argsort(key)]
    return cnt, pairs, total


def hamming_nearest(queries: torch.Tensor, refs: torch.Tensor, L: int, max_dist: int, *, want_nbest: bool = True,
                    ref_splits: int = 0):
    """Every query row against a second set of rows (barcodes against a whitelist; ss_hamming_nearest_ex):
    queries int64 [nq, q_wpr], refs int64 [nr, r_wpr] on one device, one length L.  -> (idx, dist, nbest)
    int64 [nq]: the lowest reference index at the minimum distance, that distance, and how many
    references lie at it; idx = dist = -1 (nbest 0) where no reference is within max_dist.  nbest is
    None when not wanted.  ref_splits: 0 lets the library cut the references into ranges, n forces n
    (clamped to the 32-row blocks of refs); the results are the same.  Allocates the workspace, runs on
    the current stream, makes no host sync of its own."""
    _require_cuda(queries, "queries")
    _require_cuda(refs, "refs")
    if queries.dtype != torch.int64 or refs.dtype != torch.int64 or queries.dim() != 2 or refs.dim() != 2:
        raise TypeError("queries and refs must be int64 [n, wpr] tensors")
    if refs.device != queries.device:
        raise ValueError("queries and refs must be on one device")
    dev = queries.device
    (nq, q_wpr), (nr, r_wpr) = queries.shape, refs.shape
    L_ = lib()
    ws_bytes = int(L_.ss_hamming_nearest_ws_bytes(nq, nr, L, ref_splits))
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev) if ws_bytes else None
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, dtype=torch.int32, device=dev)
    nbest = torch.empty(nq, dtype=torch.int32, device=dev) if want_nbest else None
    check(L_.ss_hamming_nearest_ex(queries.data_ptr(), nq, q_wpr, refs.data_ptr(), nr, r_wpr, L, max_dist,
                                   idx.data_ptr(), dist.data_ptr(), _ptr(nbest), _ptr(ws), ws_bytes, ref_splits,
                                   _stream(dev)), "ss_hamming_nearest_ex")
    def widen(t, none_to_minus1):     # u32 held in int32 -> int64; SS_NEAREST_NONE (0xFFFFFFFF) -> -1
        u = t.to(torch.int64) & 0xFFFFFFFF
        return torch.where(u == 0xFFFFFFFF, torch.full_like(u, -1), u) if none_to_minus1 else u
    return widen(idx, True), widen(dist, True), None if nbest is None else widen(nbest, False)


CLUSTER_METHODS = {"cluster": 0, "directional": 1, "adjacency": 3}    # SS_CLUSTER_*; 2 is not a method


def cluster_pairs(pairs: torch.Tensor, n: int, counts: Optional[torch.Tensor] = None, method: str = "directional",
                  want_sums: bool = True):
    """Group n nodes (distinct UMIs) by an undirected pair list, as UMI-tools' `cluster` (connected
    components), `directional` (edge u -> v iff c[u] >= 2 c[v] - 1) or `adjacency` method
    (ss_cluster_pairs).  `adjacency`: per component the leads are the shortest count-ordered prefix
    whose nodes and their neighbours cover it; a lead represents itself, any other node goes to its
    highest-ranked neighbour.  With rank = position by count descending, ties by index, that is
    (1) cover[v] = min rank over v and its neighbours, (2) comp[v] = the lowest rank in v's component,
    (3) thr[c] = max cover over component c, (4) v leads iff rank[v] <= thr[comp[v]], else it joins
    the node of rank cover[v].  UMI-tools leaves equal counts to set iteration order; here ties go by
    ascending index under every method.  pairs: int32 [m, 2] on the
    device, i < j, any order (hamming_all_pairs' pair output); counts: int64 [n] or None (required for
    "directional").  -> (rep int64 [n]: every node's representative, reps int64 [k]: the
    representatives by count descending, ties by index, sizes int64 [k], sums int64 [k] of the
    clusters' counts or None, rounds).  The stable descending sort of the counts is a torch call;
    the grouping runs in the HIP kernels.  Synchronises with the current stream once per round."""
    _require_cuda(pairs, "pairs")
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise TypeError("pairs must be an int32 [m, 2] tensor")
    dev = pairs.device
    m = pairs.shape[0]
    order = None
    if counts is not None:
        _require_cuda(counts, "counts")
        if counts.dtype != torch.int64 or counts.numel() != n:
            raise TypeError("counts must be an int64 [n] tensor")
        order = torch.sort(counts, descending=True, stable=True).indices.to(torch.int32)
    sums_on = want_sums and counts is not None
    L_ = lib()
    ws_bytes = int(L_.ss_cluster_ws_bytes_method(n, m, CLUSTER_METHODS[method]))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev) if sums_on else None
    ncl = torch.empty(1, dtype=torch.int64, device=dev)
    rounds = C.c_uint32(0)
    check(L_.ss_cluster_pairs(pairs.data_ptr(), m, n, _ptr(counts), _ptr(order), CLUSTER_METHODS[method], ws.data_ptr(),
                              ws_bytes, rep.data_ptr(), sizes.data_ptr(), _ptr(sums), ncl.data_ptr(), C.byref(rounds),
                              _stream(dev)), "ss_cluster_pairs")
    rep = rep.to(torch.int64) & 0xFFFFFFFF
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    by_rank = ids if order is None else order.to(torch.int64) & 0xFFFFFFFF
    reps = by_rank[rep[by_rank] == by_rank]
    if reps.numel() != int(ncl.item()):
        raise AssertionError("ss_cluster_pairs: cluster count and representatives disagree")
    return (rep, reps, sizes[reps].to(torch.int64) & 0xFFFFFFFF, sums[reps] if sums_on else None, int(rounds.value))


def umi_cluster(words: torch.Tensor, L: int, max_dist: int, counts: Optional[torch.Tensor] = None,
                method: str = "directional", pair_method: str = "auto", max_pairs_hint: Optional[int] = None):
    """UMI dedup of n distinct packed reads on the device: the pairs within `max_dist`
    (ss_hamming_all_pairs_ex, no neighbour counts, a pair buffer of max_pairs_hint -- default 4 n --
    and one more run with exactly the total when that was too small), then cluster_pairs.
    -> cluster_pairs' tuple plus the pair total."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    dev = words.device
    cap = max(1, 4 * n if max_pairs_hint is None else max_pairs_hint)
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    if n < 2:           # no pair to look for
        return cluster_pairs(torch.empty((0, 2), dtype=torch.int32, device=dev), n, counts, method) + (0,)
    while True:
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        check(lib().ss_hamming_all_pairs_ex(words.data_ptr(), n, L, wpr, max_dist, None, pairs.data_ptr(), cap,
                                            tot.data_ptr(), ALL_PAIRS_METHODS[pair_method], _stream(dev)),
              "ss_hamming_all_pairs_ex")
        total = int(tot.item())
        if total <= cap:
            break
        cap = total
    return cluster_pairs(pairs[:total], n, counts, method) + (total,)


GROUPED_ROW_TILE = 256   # rows per block of k_gp_pairs (kGpTile, csrc/ss_grouped.hip)


def _group_offsets(group_offsets, n: int, dev: torch.device) -> torch.Tensor:
    """Group offsets (a device or host tensor, or a host sequence) -> the ABI's u32 [ngroups + 1] on
    `dev`, held in an int32 tensor.  Checks first 0, nondecreasing, last n (one host read)."""
    if isinstance(group_offsets, torch.Tensor):
        if group_offsets.dtype not in (torch.int64, torch.int32):
            raise TypeError("group_offsets must be an int64 or int32 tensor, or a host sequence")
        off = group_offsets.reshape(-1).to(device=dev, dtype=torch.int64)
    else:
        off = torch.from_numpy(np.ascontiguousarray(group_offsets, dtype=np.int64).reshape(-1)).to(dev)
    if n >= 1 << 32:
        raise ValueError("n must be < 2^32")
    if off.numel() == 0:
        raise ValueError("group_offsets needs ngroups + 1 entries")
    ok = (off[0] == 0) & (off[-1] == n) & (off[1:] >= off[:-1]).all()
    if not bool(ok.item()):
        raise ValueError("group_offsets must start at 0, never decrease, and end at the number of rows")
    if off.numel() == 1 and n:
        raise ValueError("rows without a group")
    return torch.where(off >= 1 << 31, off - (1 << 32), off).to(torch.int32)      # u32 bits in int32


def hamming_all_pairs_grouped(words: torch.Tensor, L: int, max_dist: int, group_offsets, *, counts: bool = True,
                              max_pairs: int = 0):
    """hamming_all_pairs restricted to groups: rows sorted by group, group g = rows
    [group_offsets[g], group_offsets[g + 1]), only pairs inside one group are compared
    (ss_hamming_all_pairs_grouped).  -> (neighbour counts int32 [n] or None, pairs int32 [m, 2] of
    GLOBAL row indices or None, total pairs), shaped as hamming_all_pairs' result (pairs sorted, at most
    max_pairs kept; 0: count only).  group_offsets: int64 / int32 tensor on the device or a host
    sequence of ngroups + 1 entries; it is checked here (first 0, nondecreasing, last n: ValueError), which
    reads one flag back from the device; the ABI call itself does not synchronise."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    dev = words.device
    off = _group_offsets(group_offsets, n, dev)
    L_ = lib()
    ws_bytes = int(L_.ss_hamming_all_pairs_grouped_ws_bytes(n, off.numel() - 1, L))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    cnt = torch.empty(n, dtype=torch.int32, device=dev) if counts else None
    pairs = torch.empty((max(1, max_pairs), 2), dtype=torch.int32, device=dev) if max_pairs else None
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    check(L_.ss_hamming_all_pairs_grouped(words.data_ptr(), n, L, wpr, max_dist, off.data_ptr(), off.numel() - 1,
                                          _ptr(cnt), _ptr(pairs), max_pairs, tot.data_ptr(), _ptr(ws), ws_bytes,
                                          _stream(dev)), "ss_hamming_all_pairs_grouped")
    total = int(tot.item())
    if pairs is not None:
        m = min(total, max_pairs)
        p = pairs[:m].to(torch.int64)
        key = (p[:, 0] & 0xFFFFFFFF) * (1 << 32) + (p[:, 1] & 0xFFFFFFFF)
        pairs = pairs[:m][torch.argsort(key)]
    return cnt, pairs, total


def umi_cluster_grouped(words: torch.Tensor, L: int, max_dist: int, group_offsets,
                        counts: Optional[torch.Tensor] = None, method: str = "directional",
                        max_pairs_hint: Optional[int] = None):
    """UMI dedup of many groups (cell x gene, mapping position) in one call: the rows of all groups in
    one batch, sorted by group, group_offsets as in hamming_all_pairs_grouped.  The pairs inside groups
    (ss_hamming_all_pairs_grouped, no neighbour counts, a pair buffer of max_pairs_hint -- default 4 n --
    and one more run with exactly the total when that was too small), then cluster_pairs on the global
    indices: no pair crosses a group, so no cluster does, and rows of a group being contiguous, the
    (count descending, index ascending) rank restricted to a group is the group's own, so every
    representative is the one umi_cluster on that group alone would name.  "adjacency" needs nothing
    else: the global rank restricted to a group's contiguous rows is the group's own order, so leads
    and groups are those of a per-group run.
    -> cluster_pairs' tuple plus the pair total; all indices are global rows.  A cluster's group:
    ``torch.bucketize(reps, offsets[1:], right=True)``."""
    _require_cuda(words, "words")
    n, wpr = words.shape
    dev = words.device
    off = _group_offsets(group_offsets, n, dev)
    if n < 2:           # no pair to look for
        return cluster_pairs(torch.empty((0, 2), dtype=torch.int32, device=dev), n, counts, method) + (0,)
    L_ = lib()
    ngroups = off.numel() - 1
    ws_bytes = int(L_.ss_hamming_all_pairs_grouped_ws_bytes(n, ngroups, L))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    cap = max(1, 4 * n if max_pairs_hint is None else max_pairs_hint)
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    while True:
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        check(L_.ss_hamming_all_pairs_grouped(words.data_ptr(), n, L, wpr, max_dist, off.data_ptr(), ngroups, None,
                                              pairs.data_ptr(), cap, tot.data_ptr(), _ptr(ws), ws_bytes, _stream(dev)),
              "ss_hamming_all_pairs_grouped")
        total = int(tot.item())
        if total <= cap:
            break
        cap = total
    return cluster_pairs(pairs[:total], n, counts, method) + (total,)


LEN_UNDERFLOW = 0xFFFFFFFF   # ss_fastq_index: strlen 0 (the reference's size_t underflow -> too long)


def fastq_index(buf: torch.Tensor, nbytes: Optional[int] = None, *, line0: int = 0, at_eof: bool = True,
                onepass: bool = True, max_reads: Optional[int] = None):
    """Sequence lines of a FASTQ chunk resident on the device (fast_read.pyx:3-20 rule, see
    include/shortseq_amd.h ss_fastq_index) -> (offsets int64 [n], lens int64 [n], newlines).
    lens holds the reference's strlen - 1 (LEN_UNDERFLOW where strlen is 0).  The chunk must start
    at a line boundary and end right after a newline unless at_eof.
    onepass: ss_fastq_index_onepass (the chunk is read once; max_reads is a capacity guess, default
    nbytes / 16 + 2, and the call is repeated with the exact count if the chunk holds more lines);
    otherwise ss_fastq_scan + ss_fastq_index (two reads of the chunk, exact capacity)."""
    _require_cuda(buf, "buf")
    if buf.dtype != torch.uint8:
        raise TypeError("buf must be a uint8 tensor")
    nbytes = buf.numel() if nbytes is None else nbytes
    dev = buf.device
    L_ = lib()
    s = _stream(dev)
    if onepass:
        cnt = torch.empty(3, dtype=torch.int64, device=dev)
        cap = nbytes // 16 + 2 if max_reads is None else max_reads
        while True:
            ws_bytes = int(L_.ss_fastq_onepass_ws_bytes(nbytes, cap))
            ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
            offs = torch.empty(cap, dtype=torch.int64, device=dev)
            lens = torch.empty(cap, dtype=torch.int32, device=dev)
            aux = torch.empty(cap, dtype=torch.int64, device=dev)
            check(L_.ss_fastq_index_onepass(buf.data_ptr(), nbytes, line0, 1 if at_eof else 0, ws.data_ptr(), ws_bytes,
                                            offs.data_ptr(), lens.data_ptr(), aux.data_ptr(), cap, cnt.data_ptr(), s),
                  "ss_fastq_index_onepass")
            nl, n, full = (int(v) for v in cnt.tolist())
            if full:                  # a staging region ran full (lines far denser than the bound)
                cap *= 2
                continue
            if n <= cap:
                break
            cap = n
        return offs[:n], lens[:n].to(torch.int64) & 0xFFFFFFFF, nl
    ws_bytes = int(L_.ss_fastq_scan_ws_bytes(nbytes))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    check(L_.ss_fastq_scan(buf.data_ptr(), nbytes, ws.data_ptr(), ws_bytes, cnt.data_ptr(), s), "ss_fastq_scan")
    nl = int(cnt[0].item())
    cap = nl // 4 + 2
    offs = torch.empty(cap, dtype=torch.int64, device=dev)
    lens = torch.empty(cap, dtype=torch.int32, device=dev)
    aux = torch.empty(cap, dtype=torch.int64, device=dev)
    check(L_.ss_fastq_index(buf.data_ptr(), nbytes, line0, 1 if at_eof else 0, ws.data_ptr(), offs.data_ptr(),
                            lens.data_ptr(), aux.data_ptr(), cap, cnt[1:].data_ptr(), s), "ss_fastq_index")
    n = int(cnt[1].item())
    if n > cap:
        raise AssertionError("FASTQ index capacity exceeded")
    return offs[:n], lens[:n].to(torch.int64) & 0xFFFFFFFF, nl


def gather_rows(src: torch.Tensor, offsets: torch.Tensor, L: int, *, sel: Optional[torch.Tensor] = None,
                src_bytes: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense [m, round_up(L, 16)] uint8 rows gathered from a ragged byte buffer on the device:
    row r = src[offsets[sel[r]] : + L] (sel None: r).  Feeds one length group of a ragged batch to the
    fixed-length kernels."""
    _require_cuda(src, "src")
    _require_cuda(offsets, "offsets")
    if offsets.dtype != torch.int64 or (sel is not None and sel.dtype != torch.int64):
        raise TypeError("offsets / sel must be int64 tensors")
    m = (sel if sel is not None else offsets).numel()
    S = (L + 15) // 16 * 16
    if out is None:
        out = torch.empty((m, S), dtype=torch.uint8, device=src.device)
    src_bytes = src.numel() if src_bytes is None else src_bytes
    check(lib().ss_gather_rows(src.data_ptr(), src_bytes, offsets.data_ptr(), _ptr(sel), m, L, out.data_ptr(),
                               out.shape[1] if out.dim() == 2 else S, _stream(src.device)), "ss_gather_rows")
    return out


class GpuCounter:
    """Dedup counter in HBM for reads of ONE length L <= 1024 (ShortSeqCounter's hot loop,
    counter.pyx:41-54).  Counts and first-occurrence indices per distinct key: the packed word for
    L <= 32, the W = ceil(L/32) packed words for longer reads (fingerprinted, compared on words)."""

    def __init__(self, capacity: int, device=None):
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().ss_counter_create(capacity, C.byref(h)), "ss_counter_create")
        self._h = h
        self.capacity = int(lib().ss_counter_capacity(h))
        self._scratch = torch.empty(2, dtype=torch.int64, device=self.device)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ss_counter_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass

    @property
    def length(self) -> int:
        return int(lib().ss_counter_length(self._h))

    @property
    def words(self) -> int:
        """Words per key (1 for L <= 32); fixed by the first insert."""
        return int(lib().ss_counter_words(self._h))

    PASSES = ("coarse", "order", "scatter", "aggregate", "spill")

    def set_timing(self, on: bool = True) -> None:
        """Record HIP events between the partitioned insert's passes (ss_counter_set_timing)."""
        check(lib().ss_counter_set_timing(self._h, int(bool(on))), "ss_counter_set_timing")

    def pass_times(self) -> dict:
        """Mean ms per insert of each pass since the last call ({} when none was timed)."""
        ms = (C.c_double * 5)()
        k = C.c_uint64()
        check(lib().ss_counter_pass_times(self._h, ms, C.byref(k)), "ss_counter_pass_times")
        return dict(zip(self.PASSES, list(ms))) if k.value else {}

    def reset(self) -> None:
        check(lib().ss_counter_reset(self._h, _stream(self.device)), "ss_counter_reset")

    PARTITION_MIN_READS = 1 << 16   # batches at least this large reserve the partitioned path

    def reserve(self, max_reads: int) -> bool:
        """Workspace for the partitioned insert (20 B/read); False if this table cannot use it."""
        rc = lib().ss_counter_reserve(self._h, max_reads)
        return rc == 0

    def insert(self, ascii: torch.Tensor, L: Optional[int] = None, *, base_index: int = 0,
               stride: Optional[int] = None, check_errors: bool = True, partitioned: Optional[bool] = None) -> None:
        """partitioned: None = automatic (large batches), True = reserve workspace and use the
        partitioned insert if the table allows it, False = direct atomic insert."""
        n, L, stride = _as_rows(ascii, L, stride)
        if L > 32:   # multi-word keys: always partitioned, the library grows the workspace itself
            partitioned = None
        elif partitioned is None:
            partitioned = n >= self.PARTITION_MIN_READS
        if partitioned and n > int(lib().ss_counter_reserved(self._h)) and n < (1 << 32):
            self.reserve(n)
        if partitioned is False and int(lib().ss_counter_reserved(self._h)) >= n:
            self._drop_reservation()
        fb = first_bad_buffer(self.device)
        check(lib().ss_counter_insert_fixed(self._h, ascii.data_ptr(), n, L, stride, base_index,
                                            fb.data_ptr(), _stream(self.device)), "ss_counter_insert_fixed")
        if check_errors:
            _check_first_bad(fb, _fetch_row(ascii, stride, L))

    ROUTES = ("optimistic", "exact", "exact multi-word", "direct g16", "direct generic")

    def last_route(self) -> Optional[str]:
        """The kernel chain the last insert took (ss_counter_last_route; None before any insert), for
        tests that pin the dispatch: the route, then its sub-choices -- "optimistic g16 slabs",
        "exact k_pc_hist two passes", "exact multi-word one pass", "direct generic", ..."""
        code = int(lib().ss_counter_last_route(self._h))
        if code < 0:
            return None
        route = self.ROUTES[code & 7]
        if route == "optimistic":
            coarse = ("plain", "g16", "keys")[(code >> 5) & 3]
            return f"optimistic {coarse} {'slabs' if code & 128 else 'counted cursors'}"
        if route.startswith("exact"):
            hist = "" if "multi" in route else (" k_pc_keys" if code & 16 else " k_pc_hist")
            return f"{route}{hist} {'two passes' if code & 8 else 'one pass'}"
        return route

    def _drop_reservation(self) -> None:
        torch.cuda.synchronize(self.device)
        check(lib().ss_counter_release(self._h), "ss_counter_release")

    def merge(self, keys: torch.Tensor, counts: torch.Tensor, first: torch.Tensor, L: int) -> None:
        m = keys.numel()
        check(lib().ss_counter_set_length(self._h, L), "ss_counter_set_length")
        check(lib().ss_counter_merge(self._h, keys.data_ptr(), None, counts.data_ptr(), first.data_ptr(), m,
                                     _stream(self.device)), "ss_counter_merge")

    def set_spill_limit(self, reads: int) -> None:
        """Test hook (ss_counter_set_spill_limit): move the u32 slot counts into the u64 array once more
        than `reads` reads were inserted since the last spill (default 2^32 - 1)."""
        check(lib().ss_counter_set_spill_limit(self._h, int(reads)), "ss_counter_set_spill_limit")

    def size(self) -> int:
        check(lib().ss_counter_size(self._h, self._scratch.data_ptr(), _stream(self.device)), "ss_counter_size")
        return int(self._scratch[0].item())

    def overflow_word(self) -> torch.Tensor:
        """The handle's overflow word as a 1-element device tensor (no host sync)."""
        check(lib().ss_counter_overflow(self._h, self._scratch[1:].data_ptr(), _stream(self.device)),
              "ss_counter_overflow")
        return self._scratch[1:2]

    def overflowed(self) -> bool:
        return int(self.overflow_word().item()) != 0

    def extract(self, n_parts: int = 1, cap: Optional[int] = None):
        """Occupied slots grouped by owner part -> (keys, lens, counts, first, part_counts), all on
        the device; arrays sized `cap` (default: capacity + 1), valid prefix = part_counts.sum()."""
        cap = self.capacity + 1 if cap is None else cap
        d = self.device
        keys = torch.empty(cap, dtype=torch.int64, device=d)
        lens = torch.empty(cap, dtype=torch.int32, device=d)
        counts = torch.empty(cap, dtype=torch.int64, device=d)
        first = torch.empty(cap, dtype=torch.int64, device=d)
        parts = torch.empty(n_parts, dtype=torch.int64, device=d)
        check(lib().ss_counter_extract(self._h, n_parts, keys.data_ptr(), lens.data_ptr(), counts.data_ptr(),
                                       first.data_ptr(), cap, parts.data_ptr(), _stream(d)), "ss_counter_extract")
        return keys, lens, counts, first, parts

    def geometry(self):
        """(log2 capacity, log2 slots per region) of the table (region-range ownership)."""
        a, b = C.c_uint32(), C.c_uint32()
        check(lib().ss_counter_geometry(self._h, C.byref(a), C.byref(b)), "ss_counter_geometry")
        return int(a.value), int(b.value)

    def extract_ranges(self, n_parts: int, cap: Optional[int] = None):
        """As extract, with part p = the table regions owner p holds under region-range ownership
        (include/shortseq_amd.h); each part is sorted by region, the sentinel key last."""
        cap = self.capacity + 1 if cap is None else cap
        d = self.device
        keys = torch.empty(cap, dtype=torch.int64, device=d)
        lens = torch.empty(cap, dtype=torch.int32, device=d)
        counts = torch.empty(cap, dtype=torch.int64, device=d)
        first = torch.empty(cap, dtype=torch.int64, device=d)
        parts = torch.empty(n_parts, dtype=torch.int64, device=d)
        check(lib().ss_counter_extract_ranges(self._h, n_parts, keys.data_ptr(), lens.data_ptr(), counts.data_ptr(),
                                              first.data_ptr(), cap, parts.data_ptr(), _stream(d)),
              "ss_counter_extract_ranges")
        return keys, lens, counts, first, parts

    def merge_runs(self, keys: torch.Tensor, counts: torch.Tensor, first: torch.Tensor, runs, part: int,
                   n_parts: int, L: int) -> None:
        """Fold region-sorted runs (list of (begin, end) into keys / counts / first) into the regions
        this table owns as `part` of `n_parts` (ss_counter_merge_runs)."""
        d = self.device
        m = keys.numel()
        if not runs:
            return
        offs = torch.tensor([x for be in runs for x in be], dtype=torch.int64).to(d, non_blocking=True)
        log2cap, slice_log = self.geometry()
        R = 1 << (log2cap - slice_log)
        nreg = -(-(part + 1) * R // n_parts) - (-(part * R) // n_parts)
        bounds = torch.empty(len(runs) * (nreg + 1) + 1, dtype=torch.int32, device=d)
        check(lib().ss_counter_merge_runs(self._h, keys.data_ptr(), counts.data_ptr(), first.data_ptr(),
                                          offs.data_ptr(), len(runs), m, part, n_parts, L, bounds.data_ptr(),
                                          _stream(d)), "ss_counter_merge_runs")

    def pack_ranges(self, n_parts: int, skip: int = -1, first_base: int = 0, cap: Optional[int] = None):
        """Region-range parts as packed 16-B records (ss_counter_pack_ranges) -> (rec int64 [cap, 2],
        part_counts int64 [n_parts]) on the device; rec[:, 0] = key, rec[:, 1] = count | (first -
        first_base) << 32; part `skip` is left out (count 0).  Does not raise: a count or first -
        first_base that does not fit its 32-bit field sets value 4 in overflow_word(), more than cap
        records value 2; the caller checks the word (ShardedCounter sends it along the exchange)."""
        cap = self.capacity + 1 if cap is None else cap
        d = self.device
        rec = torch.empty((cap, 2), dtype=torch.int64, device=d)
        parts = torch.empty(n_parts, dtype=torch.int64, device=d)
        check(lib().ss_counter_pack_ranges(self._h, n_parts, skip, first_base, rec.data_ptr(), cap, parts.data_ptr(),
                                           _stream(d)), "ss_counter_pack_ranges")
        return rec, parts

    def merge_packed(self, rec: torch.Tensor, runs, part: int, n_parts: int, L: int) -> None:
        """Fold region-sorted packed runs (list of (begin, end, first_base) into rec) into the regions
        this table owns as `part` of `n_parts` (ss_counter_merge_packed)."""
        d = self.device
        if not runs:
            return
        m = rec.shape[0]
        offs = torch.tensor([x for (b, e, _f) in runs for x in (b, e)], dtype=torch.int64).to(d, non_blocking=True)
        bases = torch.tensor([f for (_b, _e, f) in runs], dtype=torch.int64).to(d, non_blocking=True)
        log2cap, slice_log = self.geometry()
        R = 1 << (log2cap - slice_log)
        nreg = -(-(part + 1) * R // n_parts) - (-(part * R) // n_parts)
        bounds = torch.empty(len(runs) * (nreg + 1) + 1, dtype=torch.int32, device=d)
        check(lib().ss_counter_merge_packed(self._h, rec.data_ptr(), offs.data_ptr(), bases.data_ptr(), len(runs), m,
                                            part, n_parts, L, bounds.data_ptr(), _stream(d)),
              "ss_counter_merge_packed")

    def extract_words(self, n_parts: int = 1, cap: Optional[int] = None):
        """As extract, for any key length: (fps, lens, words [cap, W], counts, first, part_counts);
        fps = the multi-word fingerprints (the packed word itself for W = 1)."""
        cap = self.capacity + 1 if cap is None else cap
        d = self.device
        W = max(1, self.words)
        fps = torch.empty(cap, dtype=torch.int64, device=d)
        lens = torch.empty(cap, dtype=torch.int32, device=d)
        words = torch.empty((cap, W), dtype=torch.int64, device=d)
        counts = torch.empty(cap, dtype=torch.int64, device=d)
        first = torch.empty(cap, dtype=torch.int64, device=d)
        parts = torch.empty(n_parts, dtype=torch.int64, device=d)
        check(lib().ss_counter_extract_words(self._h, n_parts, fps.data_ptr(), lens.data_ptr(), words.data_ptr(),
                                             counts.data_ptr(), first.data_ptr(), cap, parts.data_ptr(), _stream(d)),
              "ss_counter_extract_words")
        return fps, lens, words, counts, first, parts

    def merge_words(self, words: torch.Tensor, counts: torch.Tensor, first: torch.Tensor) -> None:
        """Fold rows of packed multi-word keys (int64 [m, W], W = the handle's words) with their counts
        and global first indices into the table (ss_counter_merge_words: keys already present add
        their counts and keep the smaller first index)."""
        m = words.shape[0]
        if m == 0:
            return
        if words.dim() != 2 or words.shape[1] != self.words:
            raise ValueError("merge_words: rows of the handle's word count")
        w, c, f = (x.contiguous() for x in (words, counts.to(torch.int64), first.to(torch.int64)))
        check(lib().ss_counter_merge_words(self._h, w.data_ptr(), c.data_ptr(), f.data_ptr(), m,
                                           _stream(self.device)), "ss_counter_merge_words")

    def items_words(self):
        """Host copy of (words u64 [m, W], counts, first) in table order (unsorted)."""
        _, _, words, counts, first, parts = self.extract_words(1)
        m = int(parts.sum().item())
        if self.overflowed():
            raise RuntimeError("GPU counter table overflowed; use a larger capacity")
        return words[:m].cpu().numpy().view(np.uint64), counts[:m].cpu().numpy(), first[:m].cpu().numpy()

    def insert_words(self, words: torch.Tensor, base_index: int = 0) -> None:
        """Count rows of already-packed keys (int64 [n, W], W = 2..64, compared whole;
        ss_counter_set_words + ss_counter_insert_words).  The first call fixes W."""
        _require_cuda(words, "words")
        if words.dim() != 2 or words.dtype != torch.int64 or not words.is_contiguous():
            raise TypeError("words: contiguous int64 [n, W]")
        check(lib().ss_counter_set_words(self._h, words.shape[1]), "ss_counter_set_words")
        check(lib().ss_counter_insert_words(self._h, words.data_ptr(), words.shape[0], base_index,
                                            _stream(self.device)), "ss_counter_insert_words")

    def items_sorted_words(self):
        """Host copy of (words u64 [m, W], counts, first) sorted by first occurrence (= dict order)."""
        _, _, words, counts, first, parts = self.extract_words(1)
        m = int(parts.sum().item())
        if self.overflowed():
            raise RuntimeError("GPU counter table overflowed; use a larger capacity")
        k = words[:m].cpu().numpy().view(np.uint64)
        c = counts[:m].cpu().numpy()
        f = first[:m].cpu().numpy()
        o = np.argsort(f, kind="stable")
        return k[o], c[o], f[o]

    def items_sorted(self):
        """Host copy of (keys u64, counts, first) sorted by first occurrence (= dict order)."""
        keys, lens, counts, first, parts = self.extract(1)
        m = int(parts.sum().item())
        if self.overflowed():
            raise RuntimeError("GPU counter table overflowed; use a larger capacity")
        k = keys[:m].cpu().numpy().view(np.uint64)
        c = counts[:m].cpu().numpy()
        f = first[:m].cpu().numpy()
        o = np.argsort(f, kind="stable")
        return k[o], c[o], f[o]
