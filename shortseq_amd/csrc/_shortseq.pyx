# cython: language_level=3, boundscheck=False, wraparound=False, cdivision=True
"""Drop-in front for the reference's Python API (shortseq/__init__.py:1-14).

Per-object operations (pack / str / ^ / == / [] on single reads) run on the host C++ codec
(csrc/host_codec.h): one read is ~tens of ns of work, a kernel launch is microseconds (SURVEY §7).
Batch operations — ShortSeqCounter over a large list, read_and_count_fastq — call the C ABI of
libshortseq_amd.so directly (include/shortseq_amd.h ss_ingest_*, bound with dlopen at the first batch call; no Python
layer, no torch): the reads are copied into the engine's pinned staging buffer (or the FASTQ file is
named), counted on the GPU, and the dict is rebuilt from the (length, words, count) rows the engine
returns in first-occurrence order.  The GPU path raises if the HIP library cannot be used, it never
degrades silently.

Object layouts match the reference so sys.getsizeof agrees (short_seq_64.pxd:11-14,
short_seq_192.pxd:11-14, short_seq_var.pxd:14-17): 32 / 48 / 32 + 8*ceil(L/32) bytes.

Documented deviations (DESIGN.md §6): hash() and the counter agree for every key (reference Q5
inserts with the raw word, so counts[pack("G"*32)] raises KeyError there); ShortSeqVar keys are
deduplicated by content (reference Q6 keys them by heap pointer).
"""
from libc.stdint cimport uint8_t, uint32_t, uint64_t, int64_t, int32_t, int16_t
from libc.string cimport memcmp, memcpy, memset, strlen
from libc.stdio cimport FILE, fopen, fclose
from libc.stdlib cimport free, malloc, calloc
from cpython.bytes cimport PyBytes_AS_STRING, PyBytes_GET_SIZE, PyBytes_FromStringAndSize
from cpython.mem cimport PyObject_Calloc, PyObject_Free
from cpython.unicode cimport PyUnicode_DecodeASCII
from cpython.object cimport PyObject
from cpython.list cimport PyList_GET_ITEM, PyList_GET_SIZE

import time

cdef extern from "Python.h":
    ctypedef Py_ssize_t Py_hash_t
    int _PyDict_SetItem_KnownHash(object mp, object key, object item, Py_hash_t hash) except -1
    PyObject* _PyDict_GetItem_KnownHash(object mp, object key, Py_hash_t hash)
    object PyUnicode_New(Py_ssize_t size, Py_UCS4 maxchar)
    void* PyUnicode_1BYTE_DATA(object o)
    void* PyUnicode_DATA(object o)
    Py_ssize_t PyUnicode_GET_LENGTH(object o)
    bint PyUnicode_Check(object o)
    bint PyBytes_Check(object o)
    bint PyBytes_CheckExact(object o)

cdef extern from "stdio.h":
    ssize_t getline(char** lineptr, size_t* n, FILE* stream) nogil

cdef extern from "shortseq_amd.h":
    ctypedef struct ss_ingest:
        pass
    enum:
        SS_ETOO_LONG
        SS_EFULL

cdef extern from "dlfcn.h":
    void* dlopen(const char* filename, int flag) nogil
    void* dlsym(void* handle, const char* symbol) nogil
    char* dlerror() nogil
    int RTLD_NOW
    int RTLD_GLOBAL

# The C ABI (include/shortseq_amd.h) bound at the first batch call, not at import: libshortseq_amd
# links the HIP runtime, and a process that imports this module before torch would otherwise map
# the system runtime first and torch its own bundled copy (two runtimes, the second sees no device).
# Loaded lazily it joins whichever runtime is already there (torch's, when torch came first).
ctypedef int (*f_device_count)(int*) noexcept nogil
ctypedef const char* (*f_last_error)() noexcept nogil
ctypedef int (*f_create)(int, ss_ingest**) noexcept nogil
ctypedef int (*f_handle)(ss_ingest*) noexcept nogil
ctypedef int (*f_staging)(ss_ingest*, uint64_t, uint8_t**) noexcept nogil
ctypedef int (*f_add_blob)(ss_ingest*, const uint8_t*, const uint32_t*, uint64_t) noexcept nogil
ctypedef int (*f_add_fastq)(ss_ingest*, const char*, uint64_t, uint64_t*) noexcept nogil
ctypedef int (*f_error)(ss_ingest*, uint64_t*, int*, uint8_t*, uint64_t, uint64_t*) noexcept nogil
ctypedef int (*f_finish)(ss_ingest*, uint64_t*, uint64_t*) noexcept nogil
ctypedef int (*f_fq_stages)(ss_ingest*, double*, uint64_t*) noexcept nogil
ctypedef int (*f_results)(ss_ingest*, const uint32_t**, const uint64_t**, const uint64_t**) noexcept nogil
ctypedef int (*f_get_device)(int*) noexcept nogil
ctypedef int (*f_fastq_split)(const char*, uint32_t, uint64_t*, uint64_t*) noexcept nogil
ctypedef int (*f_add_fastq_range)(ss_ingest*, const char*, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t*) noexcept nogil
ctypedef int (*f_set_exact)(ss_ingest*, int) noexcept nogil
ctypedef int (*f_set_adapter)(ss_ingest*, const uint8_t*, uint32_t, uint32_t, uint32_t) noexcept nogil
ctypedef int (*f_set_quality)(ss_ingest*, uint32_t, uint32_t) noexcept nogil
ctypedef int (*f_export)(ss_ingest*, uint64_t*) noexcept nogil
ctypedef int (*f_merge)(ss_ingest*, ss_ingest*, uint64_t) noexcept nogil
ctypedef int (*f_reserve_merge)(ss_ingest*, ss_ingest**, uint32_t) noexcept nogil

cdef struct _Abi:
    f_device_count device_count
    f_last_error last_error
    f_create create
    f_handle reset
    f_staging staging
    f_add_blob add_blob
    f_add_fastq add_fastq
    f_error error
    f_finish finish
    f_fq_stages fq_stages
    f_results results
    f_get_device get_device
    f_fastq_split fastq_split
    f_add_fastq_range add_fastq_range
    f_set_exact set_exact
    f_set_adapter set_adapter
    f_set_quality set_quality
    f_export export_keys
    f_merge merge
    f_reserve_merge reserve_merge

cdef _Abi _abi
cdef bint _abi_ready = False


cdef void* _sym(void* h, const char* name) except NULL:
    cdef void* p = dlsym(h, name)
    if p == NULL:
        raise ImportError(f"libshortseq_amd: missing symbol {name.decode()}")
    return p


cdef int _bind_abi() except -1:
    global _abi_ready
    if _abi_ready:
        return 0
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libshortseq_amd.so").encode()
    cdef void* h = dlopen(path, RTLD_NOW | RTLD_GLOBAL)
    if h == NULL:
        raise ImportError(f"cannot load the HIP library {path.decode()}: {dlerror().decode(errors='replace')}")
    _abi.device_count = <f_device_count>_sym(h, b"ss_device_count")
    _abi.last_error = <f_last_error>_sym(h, b"ss_last_error_string")
    _abi.create = <f_create>_sym(h, b"ss_ingest_create")
    _abi.reset = <f_handle>_sym(h, b"ss_ingest_reset")
    _abi.staging = <f_staging>_sym(h, b"ss_ingest_staging")
    _abi.add_blob = <f_add_blob>_sym(h, b"ss_ingest_add_blob")
    _abi.add_fastq = <f_add_fastq>_sym(h, b"ss_ingest_add_fastq")
    _abi.error = <f_error>_sym(h, b"ss_ingest_error")
    _abi.finish = <f_finish>_sym(h, b"ss_ingest_finish")
    _abi.results = <f_results>_sym(h, b"ss_ingest_results")
    _abi.get_device = <f_get_device>_sym(h, b"ss_get_device")
    _abi.fastq_split = <f_fastq_split>_sym(h, b"ss_fastq_split")
    _abi.add_fastq_range = <f_add_fastq_range>_sym(h, b"ss_ingest_add_fastq_range")
    _abi.set_exact = <f_set_exact>_sym(h, b"ss_ingest_set_exact")
    _abi.set_adapter = <f_set_adapter>_sym(h, b"ss_ingest_set_adapter")
    _abi.set_quality = <f_set_quality>_sym(h, b"ss_ingest_set_quality")
    _abi.export_keys = <f_export>_sym(h, b"ss_ingest_export")
    _abi.merge = <f_merge>_sym(h, b"ss_ingest_merge")
    _abi.reserve_merge = <f_reserve_merge>_sym(h, b"ss_ingest_reserve_merge")
    _abi.fq_stages = <f_fq_stages>dlsym(h, b"ss_ingest_fastq_stages")   # (optional: a bench probe)
    _abi_ready = True
    return 0

cdef extern from "host_codec.h":
    ctypedef struct ss_err:
        int32_t kind
        int32_t nbytes
        int64_t read_index
        int64_t byte_offset
    int ssh_encode "ssh::encode"(const uint8_t* s, size_t L, uint64_t* words, ss_err* err) nogil
    void ssh_decode "ssh::decode"(const uint64_t* words, size_t L, char* out) nogil
    uint64_t ssh_hamming "ssh::hamming"(const uint64_t* a, const uint64_t* b, size_t L) nogil

cdef extern from "host_trim.h":
    ctypedef struct ssh_TrimAdapter "ssh::TrimAdapter":
        pass
    bint ssh_trim_prepare "ssh::trim_prepare"(ssh_TrimAdapter* t, const uint8_t* a, uint32_t A, uint32_t min_overlap,
                                              uint32_t err_div) nogil
    uint32_t ssh_trim_read "ssh::trim_read"(const ssh_TrimAdapter& t, const uint8_t* r, uint32_t L) nogil

cdef extern from "host_qtrim.h":
    uint32_t ssh_qtrim_read "ssh::qtrim_read"(const uint8_t* q, uint32_t L, uint32_t cutoff, uint32_t base) nogil

# Domain constants (short_seq_64.pyx:27-28, short_seq_192.pyx:21-22, short_seq_var.pyx:8-10)
MIN_64_NT = 0
MAX_64_NT = 32
MIN_192_NT = 33
MAX_192_NT = 96
MIN_VAR_NT = 97
MAX_VAR_NT = 1024
DEF C_MAX_64 = 32
DEF C_MAX_192 = 96
DEF C_MAX_VAR = 1024
DEF MAX_REPR_LEN = 75

def get_domain_64(): return MIN_64_NT, MAX_64_NT
def get_domain_192(): return MIN_192_NT, MAX_192_NT
def get_domain_var(): return MIN_VAR_NT, MAX_VAR_NT


cdef inline size_t _nwords(size_t L) noexcept nogil:
    return (L + 31) // 32


cdef inline str _to_str(const uint64_t* words, size_t L):
    """_unmarshall_bytes_* (short_seq_64.pyx:114-121, short_seq_192.pyx:114-127,
    short_seq_var.pyx:98-120): decoded straight into a new compact ASCII str (no staging buffer,
    no ASCII re-validation; every character is one of "ACTG")."""
    cdef object s = PyUnicode_New(L, 127)
    if L:
        ssh_decode(words, L, <char*>PyUnicode_1BYTE_DATA(s))
    return s


cdef object _raise_encode_error(const uint8_t* seq, ss_err* err):
    """The reference's exception for a failed marshal (short_seq_64.pyx:105, util.pyx:115/137)."""
    if err.kind == 2:
        raise Exception(f"Sequences longer than {MAX_VAR_NT} bases are not supported.")
    # PyUnicode_DecodeASCII of the offending byte / 8-byte chunk; raises UnicodeDecodeError itself
    # for a non-ASCII byte, exactly as in the reference.
    cdef object bad = PyUnicode_DecodeASCII(<const char*>seq + err.byte_offset, err.nbytes, NULL)
    raise Exception(f"Unsupported base character: {bad}")


# ==================================================================================================
cdef class ShortSeq64:
    """0-32 nt: one packed word + length (short_seq_64.pyx:33-90)."""
    cdef uint64_t _packed
    cdef uint8_t _length

    def __hash__(self):
        return <Py_ssize_t>self._packed            # short_seq_64.pyx:35-36 (-1 -> -2 by CPython)

    def __len__(self):
        return self._length

    def __eq__(self, other):
        if type(other) is ShortSeq64:
            return self._length == (<ShortSeq64>other)._length and \
                   self._packed == (<ShortSeq64>other)._packed
        elif isinstance(other, (str, bytes)):
            return self._length == len(other) and str(self) == other
        return False

    def __ne__(self, other):
        return not self.__eq__(other)

    def __getitem__(self, item):
        return _getitem(&self._packed, self._length, item)

    def __xor__(self, ShortSeq64 other):
        if self._length != other._length:
            raise Exception(f"Hamming distance requires sequences of equal length "
                            f"({self._length} != {other._length})")
        return ssh_hamming(&self._packed, &other._packed, 1)

    def __str__(self):
        return _to_str(&self._packed, self._length)

    def __repr__(self):
        return f"<ShortSeq64 ({self._length} nt): {self}>"

    @property
    def packed(self):
        """The packed words as a tuple of ints (batch-layout interop)."""
        return (self._packed,)


cdef class ShortSeq192:
    """33-96 nt: three inline words + length (short_seq_192.pyx:27-97)."""
    cdef uint64_t _packed[3]
    cdef uint8_t _length

    def __hash__(self):
        return <Py_ssize_t>self._packed[0]         # short_seq_192.pyx:29-30

    def __len__(self):
        return self._length

    def __eq__(self, other):
        if type(other) is ShortSeq192:
            return self._length == (<ShortSeq192>other)._length and \
                   memcmp(self._packed, (<ShortSeq192>other)._packed, _nwords(self._length) * 8) == 0
        elif isinstance(other, (str, bytes)):
            return self._length == len(other) and str(self) == other
        return False

    def __ne__(self, other):
        return not self.__eq__(other)

    def __getitem__(self, item):
        return _getitem(self._packed, self._length, item)

    def __xor__(self, ShortSeq192 other):
        if self._length != other._length:
            raise Exception(f"Hamming distance requires sequences of equal length "
                            f"({self._length} != {other._length})")
        return ssh_hamming(self._packed, other._packed, self._length)

    def __str__(self):
        return _to_str(self._packed, self._length)

    def __repr__(self):
        return f"<ShortSeq192 ({self._length} nt): {self}>"

    @property
    def packed(self):
        return tuple(self._packed[i] for i in range(_nwords(self._length)))


cdef class ShortSeqVar:
    """97-1024 nt: heap words + length (short_seq_var.pyx:15-93)."""
    cdef uint64_t* _packed
    cdef size_t _length

    def __hash__(self):
        return <Py_ssize_t>self._packed[0]         # short_seq_var.pyx:16-17

    def __len__(self):
        return self._length

    def __eq__(self, other):
        if type(other) is ShortSeqVar:
            return self._length == (<ShortSeqVar>other)._length and \
                   memcmp(self._packed, (<ShortSeqVar>other)._packed, _nwords(self._length) * 8) == 0
        elif isinstance(other, (str, bytes)):
            return self._length == len(other) and str(self) == other
        return False

    def __ne__(self, other):
        return not self.__eq__(other)

    def __getitem__(self, item):
        return _getitem(self._packed, self._length, item)

    def __xor__(self, ShortSeqVar other):
        if self._length != other._length:
            raise Exception(f"Hamming distance requires sequences of equal length "
                            f"({self._length} != {other._length})")
        return ssh_hamming(self._packed, other._packed, self._length)

    def __str__(self):
        return _to_str(self._packed, self._length)

    def __repr__(self):
        cdef char buf[MAX_REPR_LEN]
        ssh_decode(self._packed, MAX_REPR_LEN, buf)   # short_seq_var.pyx:86-89
        return f"<ShortSeqVar ({self._length} nt): {PyUnicode_DecodeASCII(buf, MAX_REPR_LEN, NULL)} ... >"

    def __sizeof__(self):
        return sizeof(PyObject) + 16 + _nwords(self._length) * 8   # short_seq_var.pyx:83-84

    def __dealloc__(self):
        if self._packed is not NULL:
            PyObject_Free(self._packed)

    @property
    def packed(self):
        return tuple(self._packed[i] for i in range(_nwords(self._length)))


# Singleton (short_seq.pyx:7)
cdef ShortSeq64 empty = ShortSeq64.__new__(ShortSeq64)


# ==================================================================================================
# Construction (short_seq.pyx:13-74)
cdef object _new(const uint8_t* seq, size_t length):
    cdef ss_err err
    cdef ShortSeq64 o64
    cdef ShortSeq192 o192
    cdef ShortSeqVar ovar
    cdef uint64_t* words
    if length == 0:
        return empty
    elif length <= C_MAX_64:
        o64 = ShortSeq64.__new__(ShortSeq64)
        if ssh_encode(seq, length, &o64._packed, &err):
            _raise_encode_error(seq, &err)
        o64._length = <uint8_t>length
        return o64
    elif length <= C_MAX_192:
        o192 = ShortSeq192.__new__(ShortSeq192)
        if ssh_encode(seq, length, o192._packed, &err):
            _raise_encode_error(seq, &err)
        o192._length = <uint8_t>length
        return o192
    elif length <= C_MAX_VAR:
        words = <uint64_t*>PyObject_Calloc(_nwords(length), sizeof(uint64_t))
        if words is NULL:
            raise MemoryError(f"Error while allocating new ShortSeq of length {length}.")
        if ssh_encode(seq, length, words, &err):
            PyObject_Free(words)
            _raise_encode_error(seq, &err)
        ovar = ShortSeqVar.__new__(ShortSeqVar)
        ovar._packed = words
        ovar._length = length
        return ovar
    raise Exception(f"Sequences longer than {MAX_VAR_NT} bases are not supported.")


cdef object _from_words(const uint64_t* w, size_t length):
    """Object for already-packed words (batch results -> drop-in objects)."""
    cdef ShortSeq64 o64
    cdef ShortSeq192 o192
    cdef ShortSeqVar ovar
    if length == 0:
        return empty
    if length <= C_MAX_64:
        o64 = ShortSeq64.__new__(ShortSeq64)
        o64._packed = w[0]
        o64._length = <uint8_t>length
        return o64
    if length <= C_MAX_192:
        o192 = ShortSeq192.__new__(ShortSeq192)
        memcpy(o192._packed, w, _nwords(length) * 8)
        o192._length = <uint8_t>length
        return o192
    ovar = ShortSeqVar.__new__(ShortSeqVar)
    ovar._packed = <uint64_t*>PyObject_Calloc(_nwords(length), sizeof(uint64_t))
    if ovar._packed is NULL:
        raise MemoryError()
    memcpy(ovar._packed, w, _nwords(length) * 8)
    ovar._length = length
    return ovar


def from_words(words, size_t length):
    """Build a ShortSeq from packed words (sequence of ints)."""
    cdef uint64_t buf[32]
    cdef size_t i, n = _nwords(length)
    if length > C_MAX_VAR:
        raise Exception(f"Sequences longer than {MAX_VAR_NT} bases are not supported.")
    memset(buf, 0, sizeof(buf))
    for i in range(n):
        buf[i] = <uint64_t>(int(words[i]) & 0xFFFFFFFFFFFFFFFF)
    return _from_words(buf, length)


cdef inline object _from_py_str(str s):
    # short_seq.pyx:40-43: the raw PyUnicode buffer, length in code points (SURVEY: UCS-2 quirk kept)
    return _new(<const uint8_t*>PyUnicode_DATA(s), <size_t>PyUnicode_GET_LENGTH(s))


cdef inline object _from_py_bytes(bytes b):
    return _new(<const uint8_t*>PyBytes_AS_STRING(b), <size_t>PyBytes_GET_SIZE(b))


def pack(seq, /):
    """short_seq.pyx:13-28."""
    if PyUnicode_Check(seq):
        if not seq:
            return empty
        return _from_py_str(seq)
    elif PyBytes_Check(seq):
        if not seq:
            return empty
        return _from_py_bytes(seq)
    elif type(seq) is ShortSeq64 or type(seq) is ShortSeq192 or type(seq) is ShortSeqVar:
        return seq
    raise TypeError(f'Cannot pack objects of type "{type(seq)}"')


def from_str(str seq_str):
    if not seq_str:
        return empty
    return _from_py_str(seq_str)


def from_bytes(bytes seq_bytes):
    if not seq_bytes:
        return empty
    return _from_py_bytes(seq_bytes)


# ==================================================================================================
# Subscript / slice (short_seq.pyx:78-238, short_seq_64.pyx:53-75): bit-exact funnel-shift copy of
# nts [start, start + n), trimmed to 2n bits.
cdef object _slice_words(const uint64_t* src, size_t start, size_t n):
    cdef uint64_t buf[32]
    cdef size_t bit = 2 * start, nw = _nwords(n), i, w, o
    cdef size_t tail = (2 * n) % 64
    memset(buf, 0, sizeof(buf))
    w = bit // 64
    o = bit % 64
    for i in range(nw):
        if o == 0:
            buf[i] = src[w + i]
        else:
            buf[i] = src[w + i] >> o
            if (w + i + 1) * 32 < start + n:       # only words that hold nts of the slice
                buf[i] |= src[w + i + 1] << (64 - o)
    if tail:
        buf[nw - 1] &= (1ULL << tail) - 1
    return _from_words(buf, n)


cdef object _getitem(const uint64_t* packed, size_t length, item):
    cdef Py_ssize_t index, start, stop, step, slen
    cdef ShortSeq64 one
    if isinstance(item, slice):
        start, stop, step = item.indices(length)
        if step != 1:
            raise TypeError("Slice step not supported")
        slen = stop - start if stop > start else 0
        if slen == 0:
            return empty
        return _slice_words(packed, start, slen)
    elif isinstance(item, int):
        index = item
        if index < 0:
            index += length
        if index < 0 or index >= <Py_ssize_t>length:
            raise IndexError("Sequence index out of range")
        one = ShortSeq64.__new__(ShortSeq64)
        one._packed = (packed[index // 32] >> (2 * (index % 32))) & 3
        one._length = 1
        return one
    raise TypeError(f"Invalid index type: {type(item)}")


# ==================================================================================================
# Counter (counter.pyx:10-70)
GPU_MIN_READS = 1 << 16     # below this a list is counted on the host (launch + copy overhead)


cdef class ShortSeqCounter(dict):
    """dict subclass {ShortSeq: count} in first-occurrence order (counter.pyx:10-54).

    ShortSeqCounter(list_of_bytes, device="auto"): lists of >= GPU_MIN_READS reads are encoded and
    counted on the GPU (ss_ingest: split on the device into lengths 1-32 and length classes 33-1024,
    counter tables keyed by (length, words): lengths 1-31 in one, 32 in one, a class each);
    device="host" forces the per-object host path, device="cuda"/"cuda:N" forces the GPU.
    """

    def __init__(self, source=None, device="auto"):
        super().__init__()
        if type(source) is list:                    # counter.pyx:14: only lists are consumed
            self._count_list(source, device)

    def __setitem__(self, key, val):
        if type(key) not in (ShortSeq64, ShortSeq192, ShortSeqVar):
            raise TypeError(f"{self.__class__} does not support {type(key)} keys")
        dict.__setitem__(self, key, val)

    cdef _count_list(self, list it, device):
        cdef Py_ssize_t n = PyList_GET_SIZE(it)
        devs = []
        if device != "host" and n >= (GPU_MIN_READS if device == "auto" else 0):
            devs = _resolve_devices(device)
        if devs:
            _count_batch_gpu(self, it, devs)
        else:
            self._count_host(it)

    cdef _count_host(self, list it):
        cdef Py_ssize_t i, n = PyList_GET_SIZE(it)
        cdef object item, seq
        for i in range(n):
            item = <object>PyList_GET_ITEM(it, i)
            if not PyBytes_CheckExact(item):
                raise TypeError(f"expected bytes, {type(item).__name__} found")
            seq = _from_py_bytes(item)
            dict.__setitem__(self, seq, dict.get(self, seq, 0) + 1)


def _current_device():
    """The caller's current device: torch's when torch has initialised HIP (its current device is
    what a multi-rank job sets per rank), else the HIP runtime's for this thread."""
    import sys
    cdef int d = 0
    t = sys.modules.get("torch")
    if t is not None:
        try:
            if t.cuda.is_initialized():
                return int(t.cuda.current_device())
        except Exception:  # noqa: BLE001
            pass
    if _abi.get_device(&d) != 0:
        return 0
    return d


def _resolve_devices(device):
    """device argument -> the HIP devices a batch call shards over (contiguous read ranges, in
    order), or [] for the host path.
      "host"                 the reference's per-object loop
      "auto"                 the caller's current device only (ADVICE r3: a worker of an mpirun /
                             srun / multiprocessing job must not open engines on every GPU of the
                             node); the host path when no HIP runtime / device is usable.  Fan-out
                             over several devices is opt-in: "all" or a list
      "cuda"                 the current device
      "cuda:N" / torch.device("cuda", N) / N      device N
      "all"                  every visible device
      a list / tuple of the above                 those devices, in that order (one engine each; a
                                                  device may repeat)"""
    cdef int count = 0
    if isinstance(device, str) and device == "host":
        return []
    if isinstance(device, str) and device == "auto":
        try:
            _bind_abi()
        except ImportError:
            return []
        if _abi.device_count(&count) != 0 or count <= 0:
            return []
        return [_current_device()]
    _bind_abi()
    if _abi.device_count(&count) != 0 or count <= 0:
        raise RuntimeError(f"shortseq_amd: device {device!r} requested but no HIP device is visible")
    if isinstance(device, (list, tuple)):
        out = []
        for d in device:
            out.extend(_resolve_devices(d))
        if not out:
            raise ValueError("empty device list")
        return out
    if isinstance(device, int):
        idx = device
    else:
        name = str(device)
        if name == "cuda":
            return [_current_device()]
        if name == "all":
            return list(range(count))
        if not name.startswith("cuda:"):
            raise ValueError(f"unknown device {device!r} (use 'auto', 'host', 'cuda', 'cuda:N', 'all' or a list)")
        idx = int(name[5:])
    if idx < 0 or idx >= count:
        raise ValueError(f"device {device!r}: {count} HIP device(s) visible")
    return [idx]


# Ingest engines: a pool of idle engines per device.  A call takes one engine per shard and gives
# them back when its dict is built, so concurrent calls from several Python threads (the GIL is
# released while they count) never share an engine, its pinned staging or its result buffers.
import threading
_pool_lock = threading.Lock()
cdef dict _idle_engines = {}


cdef ss_ingest* _engine(int dev) except NULL:
    """An idle engine of device `dev` (reset), or a new one."""
    cdef ss_ingest* g = NULL
    cdef size_t h = 0
    cdef int rc
    with _pool_lock:
        lst = _idle_engines.get(dev)
        if lst:
            h = lst.pop()
    if h:
        g = <ss_ingest*>h
        rc = _abi.reset(g)
    else:
        rc = _abi.create(dev, &g)
    if rc != 0:
        raise RuntimeError(f"shortseq_amd GPU engine: {_abi.last_error().decode(errors='replace')} (rc {rc})")
    return g


cdef _engine_release(int dev, ss_ingest* g):
    with _pool_lock:
        _idle_engines.setdefault(dev, []).append(<size_t>g)


cdef _ingest_check(int rc, what):
    if rc != 0:
        raise RuntimeError(f"shortseq_amd {what}: {_abi.last_error().decode(errors='replace')} (rc {rc})")


cdef _raise_ingest_error(ss_ingest* g):
    """The first rejected read, as the reference raises it (the host codec re-encodes its bytes)."""
    cdef uint64_t idx = 0, ln = 0
    cdef int kind = 0
    _ingest_check(_abi.error(g, &idx, &kind, NULL, 0, &ln), "ingest error")
    if idx == <uint64_t>-1:
        return
    if kind == SS_ETOO_LONG:
        raise Exception(f"Sequences longer than {MAX_VAR_NT} bases are not supported.")
    buf = PyBytes_FromStringAndSize(NULL, ln)
    _ingest_check(_abi.error(g, &idx, &kind, <uint8_t*>PyBytes_AS_STRING(buf), ln, &ln), "ingest error")
    _from_py_bytes(buf)          # raises the reference's exception for this read
    raise RuntimeError("ingest flagged a read the host codec accepts")   # not reached


cdef _fill_rows(ShortSeqCounter self, uint64_t K, const uint32_t* lens, const uint64_t* counts,
                const uint64_t* words):
    """Insert the engine's rows (distinct keys in first-occurrence order) into the empty dict: one key
    object per row, inserted with its known hash (the objects' own __hash__ = packed word 0, -1 ->
    -2; counter.pyx:44-50 inserts the same way), so the loop walks the arrays front to back with no
    per-key __hash__ call, lookup, tuple or sort.  A call sharded over several engines reaches here
    once, with the shards already reduced on the devices (ss_ingest_merge)."""
    cdef uint64_t k, woff = 0
    cdef uint32_t L
    cdef Py_hash_t h
    for k in range(K):
        L = lens[k]
        if L == 0:
            dict.__setitem__(self, empty, counts[k])
            continue
        h = <Py_hash_t>words[woff]
        if h == -1:
            h = -2
        _PyDict_SetItem_KnownHash(self, _from_words(words + woff, L), counts[k], h)
        woff += _nwords(L)


def _fill_from_arrays(ShortSeqCounter counter, lens, counts, words):
    """Host-side test hook for the dict rebuild: numpy arrays in the ss_ingest_results layout."""
    import numpy as np
    cdef uint32_t[::1] lv = np.ascontiguousarray(lens, dtype=np.uint32)
    cdef uint64_t[::1] cv = np.ascontiguousarray(counts, dtype=np.uint64)
    cdef uint64_t[::1] wv = np.ascontiguousarray(np.concatenate([np.asarray(words, np.uint64), np.zeros(1, np.uint64)]))
    _fill_rows(counter, lv.shape[0], &lv[0] if lv.shape[0] else NULL, &cv[0] if cv.shape[0] else NULL, &wv[0])


cdef _fill_from_engine(ShortSeqCounter self, ss_ingest* g):
    """The rows of a finished engine (its first rejected read raises instead)."""
    cdef const uint32_t* lens
    cdef const uint64_t* counts
    cdef const uint64_t* words
    _raise_ingest_error(g)
    _ingest_check(_abi.results(g, &lens, &counts, &words), "ingest results")
    _fill_rows(self, _engine_keys(g), lens, counts, words)


_REDUCE_MODE = "auto"


def _set_reduce_mode(str mode):
    """Test / probe hook: "tree" (default) or "chain" (every shard merged into engine 0 in turn)."""
    global _REDUCE_MODE
    if mode not in ("auto", "tree", "chain"):
        raise ValueError(mode)
    _REDUCE_MODE = mode


def _merge_pair(size_t ga, size_t gb, uint64_t rel_base, bint reexport):
    """Engine b's entries folded into engine a (ss_ingest_merge on a's device and stream; b's reads
    follow a's from a-relative index rel_base on).  reexport: b received merges of its own since its
    export, so its tables are extracted again first."""
    cdef ss_ingest* a = <ss_ingest*>ga
    cdef ss_ingest* b = <ss_ingest*>gb
    cdef uint64_t K = 0
    cdef int rc = 0
    with nogil:
        if reexport:
            rc = _abi.export_keys(b, &K)
        if rc == 0:
            rc = _abi.merge(a, b, rel_base)
    _ingest_check(rc, "ingest merge")


cdef _reduce_fill(ShortSeqCounter self, list engines, list bases):
    """The dict of a call counted on len(engines) shards (engine k: the reads from bases[k] on).  The
    first rejected read in input order raises (shard order = input order).  Shards on distinct
    devices reduce on the devices as a tree (VERDICT r4 item 5): round r merges engine k + 2^r into
    engine k for every k divisible by 2^(r+1), the round's merges concurrently, each on its
    destination's device and stream (ss_ingest_merge: peer copies over xGMI) -- so no engine takes
    more than log2(D) sources and the first round's D/2 copies use D/2 links at once.  Shards that all
    share one device reduce as a chain into engine 0: there the tree's concurrent merges share one
    GPU and its re-exports are extra work (tools/probe_reduce.py, profiles/r5: 8 x 2^24 keys, chain
    30 ms vs tree 49 ms).  Every pair is adjacent in input order
    (b's reads follow a's), which keeps the smallest row of a key its first occurrence.  Engine 0 then
    orders the union by first read (ss_ingest_finish), and the dict is built once from those rows --
    each distinct key crosses PCIe once and gets one dict insert."""
    cdef Py_ssize_t k, D = len(engines)
    cdef ss_ingest* g0 = <ss_ingest*><size_t>engines[0][1]
    cdef uint64_t K = 0, NW = 0
    cdef int rc = 0
    for k in range(D):
        _raise_ingest_error(<ss_ingest*><size_t>engines[k][1])
    if D > 1:
        mode = _REDUCE_MODE
        if mode == "auto":
            mode = "chain" if len(set(e[0] for e in engines)) == 1 else "tree"
        if mode == "chain":
            _reserve_merge(<size_t>engines[0][1], [<size_t>engines[k][1] for k in range(1, D)])
            for k in range(1, D):
                _merge_pair(<size_t>engines[0][1], <size_t>engines[k][1], bases[k], False)
        else:
            # every destination sized once for the union of the engines it will absorb (a absorbs
            # a + 1 .. a + lowbit(a) - 1; engine 0 all others).  One after another: a reserve reads
            # its sources' bin maps while another destination's reserve may add bins to them
            # (ADVICE r5: concurrent reserves raced on a std::map); they are cheap next to the merges
            for a in range(0, D, 2):
                span = (a & -a) if a else D
                srcs = [<size_t>engines[b][1] for b in range(a + 1, min(D, a + span))]
                if srcs:
                    _reserve_merge(<size_t>engines[a][1], srcs)
            step = 1
            while step < D:
                pairs = [(a, a + step) for a in range(0, D, 2 * step) if a + step < D]
                # b merged sources of its own in an earlier round (b + step/2 .. ): re-export it
                jobs = [(<size_t>engines[a][1], <size_t>engines[b][1], <uint64_t>(bases[b] - bases[a]),
                         step > 1 and b + 1 < D) for a, b in pairs]
                _run_parallel(_merge_pair, jobs)
                step *= 2
        with nogil:
            rc = _abi.finish(g0, &K, &NW)
        _ingest_check(rc, "ingest finish")
        _engine_nkeys[<size_t>g0] = K
    _fill_from_engine(self, g0)


def _reserve_merge(size_t gd, list srcs):
    """Destination gd's tables and row maps sized once for the union of the (exported) sources'
    entries (ss_ingest_reserve_merge), so its merges do not grow the tables one merge at a time."""
    cdef ss_ingest* d = <ss_ingest*>gd
    cdef uint32_t k, n = len(srcs)
    cdef ss_ingest** arr = <ss_ingest**>malloc(max(1, n) * sizeof(ss_ingest*))
    cdef int rc = 0
    if arr == NULL:
        raise MemoryError()
    try:
        for k in range(n):
            arr[k] = <ss_ingest*><size_t>srcs[k]
        with nogil:
            rc = _abi.reserve_merge(d, arr, n)
    finally:
        free(arr)
    _ingest_check(rc, "ingest reserve merge")


def _run_parallel(fn, jobs):
    """fn(*job) for every job, all but the first in threads (the GIL is released inside); the first
    exception raised is re-raised after every job ended."""
    errs = [None] * len(jobs)

    def run(i):
        try:
            fn(*jobs[i])
        except BaseException as e:  # noqa: BLE001
            errs[i] = e
    ts = [threading.Thread(target=run, args=(i,)) for i in range(1, len(jobs))]
    for t in ts:
        t.start()
    if jobs:
        run(0)
    for t in ts:
        t.join()
    for e in errs:
        if e is not None:
            raise e


cdef dict _engine_nkeys = {}


cdef uint64_t _engine_keys(ss_ingest* g):
    return _engine_nkeys.get(<size_t>g, 0)


def _shard_work(size_t gh, int kind, size_t blob, size_t lens, uint64_t n, bytes path, uint64_t begin,
                uint64_t end, uint64_t line0, uint64_t chunk, size_t nseqs_p, bint export):
    """One shard on its engine, GIL released: count (a staged list slice, or a FASTQ byte range),
    then -- unless it holds a rejected read -- finish (its rows into the engine's pinned results), or
    with `export` (one shard of several) extract its tables for the device-side reduce."""
    cdef ss_ingest* g = <ss_ingest*>gh
    cdef int rc, bad_kind = 0
    cdef uint64_t bad_idx = 0, K = 0, NW = 0
    cdef uint64_t* nseqs = <uint64_t*>nseqs_p
    cdef const char* cpath = NULL
    if kind == 1:
        cpath = path
    with nogil:
        if kind == 0:
            rc = _abi.add_blob(g, <const uint8_t*>blob, <const uint32_t*>lens, n)
        else:
            rc = _abi.add_fastq_range(g, cpath, begin, end, line0, chunk, nseqs)
        if rc == SS_EFULL:
            # a length class's table, sized by its distinct-key sketch, ran full (the sketch
            # under-estimated): the shard is counted again with tables sized by their rows
            rc = _abi.reset(g)
            if rc == 0:
                rc = _abi.set_exact(g, 1)
            if rc == 0:
                if kind == 0:
                    rc = _abi.add_blob(g, <const uint8_t*>blob, <const uint32_t*>lens, n)
                else:
                    rc = _abi.add_fastq_range(g, cpath, begin, end, line0, chunk, nseqs)
            _abi.set_exact(g, 0)
        if rc == 0:
            rc = _abi.error(g, &bad_idx, &bad_kind, NULL, 0, NULL)
        if rc == 0 and bad_idx == <uint64_t>-1:
            if export:
                rc = _abi.export_keys(g, &K)
            else:
                rc = _abi.finish(g, &K, &NW)
    _ingest_check(rc, "ingest")
    _engine_nkeys[gh] = K


def _run_shards(jobs):
    """jobs: argument tuples of _shard_work, one per engine; all but the first run in threads."""
    _run_parallel(_shard_work, jobs)


def _count_batch_gpu(ShortSeqCounter self, list reads, devs):
    """Batch path (counter.pyx:22-39 over a whole list): the list is cut into len(devs) contiguous
    shards; each shard's bytes objects are copied back to back into its engine's pinned staging
    buffer and counted on that engine's device (split on the device into lengths 1-32 and length
    classes, tables keyed by length and words (lengths 1-31 share one): the length is part of the key, short_seq_64.pyx:41-44),
    the shards concurrently.  Several shards reduce on the devices into the first shard's engine
    (_reduce_fill: ss_ingest_export + ss_ingest_merge), which orders the union by global first read
    -- the first-occurrence order of the whole list.  The first rejected read in list order raises
    the reference's error."""
    cdef Py_ssize_t i, n = PyList_GET_SIZE(reads), ln
    cdef uint64_t total = 0, sub
    cdef object item
    cdef uint8_t* dst
    cdef uint8_t* base
    cdef uint32_t* lens = <uint32_t*>malloc(max(1, n) * sizeof(uint32_t))
    cdef ss_ingest* g
    cdef Py_ssize_t D, k, lo, hi
    cdef uint64_t nseq = 0
    if lens == NULL:
        raise MemoryError()
    engines = []
    try:
        for i in range(n):
            item = <object>PyList_GET_ITEM(reads, i)
            if not PyBytes_CheckExact(item):
                # the host loop would raise here unless an earlier read is invalid: find out first
                _raise_first_error(reads, i)
                raise TypeError(f"expected bytes, {type(item).__name__} found")
            ln = PyBytes_GET_SIZE(item)
            lens[i] = <uint32_t>ln if ln < 0xFFFFFFFF else <uint32_t>0xFFFFFFFF
            total += ln
        D = max(1, min(len(devs), n))
        jobs = []
        for k in range(D):
            lo, hi = n * k // D, n * (k + 1) // D
            g = _engine(devs[k])
            engines.append((devs[k], <size_t>g))
            sub = 0
            for i in range(lo, hi):
                sub += lens[i]
            _ingest_check(_abi.staging(g, sub, &base), "ingest staging")
            dst = base
            for i in range(lo, hi):
                ln = lens[i]
                memcpy(dst, PyBytes_AS_STRING(<object>PyList_GET_ITEM(reads, i)), ln)
                dst += ln
            jobs.append((<size_t>g, 0, <size_t>base, <size_t>(lens + lo), <uint64_t>(hi - lo), b"", 0, 0, 0, 0, None))
        _run_shard_jobs(jobs)
        _reduce_fill(self, engines, [n * k // D for k in range(D)])
    finally:
        free(lens)
        for d, h in engines:
            _engine_nkeys.pop(h, None)
            _engine_release(d, <ss_ingest*><size_t>h)


def _run_shard_jobs(jobs):
    """_run_shards with the nseqs out-pointer of every FASTQ job owned here; several jobs export
    their tables for the device-side reduce instead of finishing."""
    cdef uint64_t* ns = <uint64_t*>calloc(max(1, len(jobs)), sizeof(uint64_t))
    if ns == NULL:
        raise MemoryError()
    cdef Py_ssize_t i
    cdef size_t base = <size_t>ns
    try:
        full = []
        for i in range(len(jobs)):
            full.append((*jobs[i][:10], base + 8 * i, len(jobs) > 1))
        _run_shards(full)
        return [ns[i] for i in range(len(jobs))]
    finally:
        free(ns)


def _raise_first_error(list reads, Py_ssize_t upto):
    """Re-run the reference's loop on reads[0:upto] (host codec) so the first failure raises exactly
    the exception the reference raises."""
    cdef Py_ssize_t i
    cdef object item
    for i in range(upto):
        item = <object>PyList_GET_ITEM(reads, i)
        if not PyBytes_CheckExact(item):
            raise TypeError(f"expected bytes, {type(item).__name__} found")
        _from_py_bytes(item)


cdef bytes _adapter_arg(adapter, min_overlap, err_div):
    """The adapter option of read_and_count_fastq as bytes, checked as the C ABI checks it."""
    if isinstance(adapter, str):
        adapter = adapter.encode("ascii")
    if not isinstance(adapter, bytes):
        raise TypeError(f"adapter: bytes or str expected, {type(adapter).__name__} found")
    if not 1 <= len(adapter) <= 64:
        raise ValueError("adapter of 1 .. 64 bytes expected")
    if min_overlap < 1:
        raise ValueError("min_overlap >= 1 expected")
    if err_div < 0:
        raise ValueError("err_div >= 0 expected")
    return adapter


def read_and_count_fastq(filename, device="auto", *, adapter=None, min_overlap=3, err_div=10, quality_cutoff=None,
                         quality_base=33, _chunk_bytes=0):
    """counter.pyx:57-70 + fast_read.pyx:3-20: keep line 2 of every 4 lines; each kept line loses
    exactly its last character (strlen - 1, short_seq.pyx:50-52); prints the reference's timings.
    device "auto" (the current GPU) / "cuda[:N]" / "all" / a list: the file is cut into one byte
    range per device at line boundaries (ss_fastq_split), each range streamed to its device in
    pinned chunks and indexed, split by length and counted there (ss_ingest_add_fastq_range), the
    ranges concurrently, and the dict built from the ranges' rows in file order; "host": the
    reference's per-line loop.
    adapter (bytes or str, 1..64 bytes, 'N' = wildcard; keyword-only, not in the reference): every
    sequence line is cut at the leftmost position where the adapter matches with an overlap of at
    least min_overlap and at most overlap // err_div mismatches (no indels, not best-scoring;
    include/shortseq_amd.h, "3' adapter trim") before it is counted -- on the device for the GPU paths,
    with csrc/host_trim.h for "host".  A read is judged on its kept prefix only.
    quality_cutoff (1..93; keyword-only, not in the reference) with quality_base (33 or 64): before the
    adapter cut every sequence line loses its low-quality 3' end by BWA's running-sum rule over the
    record's quality line (include/shortseq_amd.h, "3' quality trim") -- on the device for the GPU
    paths, with csrc/host_qtrim.h for "host".  A record whose quality line is missing or shorter than
    its sequence line keeps its length."""
    import os
    cdef bytes ad = None if adapter is None else _adapter_arg(adapter, min_overlap, err_div)
    cdef ssh_TrimAdapter trim
    cdef uint32_t qc = 0, qb = 33
    if quality_cutoff is not None:
        if not 1 <= quality_cutoff <= 93:
            raise ValueError("quality_cutoff in 1 .. 93 expected")
        if quality_base not in (33, 64):
            raise ValueError("quality_base of 33 or 64 expected")
        qc = quality_cutoff
        qb = quality_base
    devs = _resolve_devices(device)
    if devs:
        return _read_and_count_fastq_gpu(filename, devs, _chunk_bytes, ad, min_overlap, err_div, qc, qb)
    if ad is not None:
        ssh_trim_prepare(&trim, <const uint8_t*>PyBytes_AS_STRING(ad), <uint32_t>len(ad), min_overlap, err_div)
    cdef FILE* f
    cdef char* line = NULL
    cdef size_t cap = 0
    cdef ssize_t got
    cdef size_t count = 1
    cdef size_t ln
    cdef size_t qn
    cdef bytes held = None        # with a cutoff: the sequence line that waits for its quality line
    seqs = []
    t1 = time.time()
    fname = filename.encode("utf-8")
    f = fopen(fname, "rb")
    if f == NULL:
        raise Exception(f"{str(fname)}: Something went wrong while reading this file.")
    try:
        while True:
            got = getline(&line, &cap, f)
            if got == -1:
                break
            if count % 2 == 0 and count % 4 != 0:
                ln = strlen(line)
                if ln == 0:   # strlen - 1 underflows in the reference -> the too-long error
                    raise Exception(f"Sequences longer than {MAX_VAR_NT} bases are not supported.")
                ln -= 1
                if qc:
                    held = PyBytes_FromStringAndSize(line, ln)
                else:
                    if ad is not None and ln <= C_MAX_VAR:
                        ln = ssh_trim_read(trim, <const uint8_t*>line, <uint32_t>ln)
                    seqs.append(PyBytes_FromStringAndSize(line, ln))
            elif held is not None and count % 4 == 0:
                # the quality line as it stands in the file: every byte up to its newline, NULs included
                ln = len(held)
                qn = <size_t>got - (1 if line[got - 1] == b'\n' else 0)
                if ln <= C_MAX_VAR and qn >= ln:
                    ln = ssh_qtrim_read(<const uint8_t*>line, <uint32_t>ln, qc, qb)
                if ad is not None and ln <= C_MAX_VAR:
                    ln = ssh_trim_read(trim, <const uint8_t*>PyBytes_AS_STRING(held), <uint32_t>ln)
                seqs.append(held[:ln])
                held = None
            count += 1
        if held is not None:      # the file ended before the record's quality line: the read keeps its length
            ln = len(held)
            if ad is not None and ln <= C_MAX_VAR:
                ln = ssh_trim_read(trim, <const uint8_t*>PyBytes_AS_STRING(held), <uint32_t>ln)
            seqs.append(held[:ln])
    finally:
        fclose(f)
        free(line)
    t2 = time.time()
    counts = ShortSeqCounter(seqs, device="host")
    t3 = time.time()
    print(f"{t2-t1:.2f}s to read {len(seqs)} total seqs, and {t3 - t2:.2f}s to count {len(counts)} unique sequences")
    return counts


_last_fastq_stages = []    # the last GPU call's stage split, per device (fastq_stage_times)


def fastq_stage_times():
    """Stage split of the last GPU read_and_count_fastq call, one dict per device (ms; bench / probes):
    file reads into pinned memory, device H2D (summed pieces, overlapping the reads), index, count,
    finish, bytes copied; on the first, the reduce + dict build and the whole call."""
    return [dict(x) for x in _last_fastq_stages]


def _read_and_count_fastq_gpu(filename, devs, uint64_t chunk_bytes=0, bytes adapter=None, uint32_t min_overlap=3,
                              uint32_t err_div=10, uint32_t quality_cutoff=0, uint32_t quality_base=33):
    """The file streamed through one engine per device: range k of ss_fastq_split on devs[k]
    (parallel preads into pinned staging, chunks ending after a newline, one-read FASTQ index, split
    by length and counted on the device); the ranges reduced on the devices in range order
    (_reduce_fill).  With `adapter` every engine taken trims its chunks' lengths after the index
    (ss_ingest_set_adapter), and with `quality_cutoff` lowers them before that (ss_ingest_set_quality);
    the engines are pooled, so both settings are cleared before they go back."""
    import os
    cdef int rc
    cdef Py_ssize_t D = len(devs), k
    fname = filename.encode("utf-8")
    if not os.path.isfile(filename):
        raise Exception(f"{str(fname)}: Something went wrong while reading this file.")
    cdef uint64_t* begin = <uint64_t*>calloc(D + 1, sizeof(uint64_t))
    cdef uint64_t* line0 = <uint64_t*>calloc(D + 1, sizeof(uint64_t))
    cdef double st_ms[5]
    cdef uint64_t st_bytes = 0
    stages = []
    if begin == NULL or line0 == NULL:
        free(begin)
        free(line0)
        raise MemoryError()
    engines = []
    t1 = time.time()
    try:
        if D > 1:
            _ingest_check(_abi.fastq_split(fname, <uint32_t>D, begin, line0), "fastq split")
        else:
            begin[1] = <uint64_t>-1
        jobs = []
        for k in range(D):
            g = <size_t>_engine(devs[k])
            engines.append((devs[k], g))
            if adapter is not None:
                _ingest_check(_abi.set_adapter(<ss_ingest*><size_t>g, <const uint8_t*>PyBytes_AS_STRING(adapter),
                                               <uint32_t>len(adapter), min_overlap, err_div), "ingest set adapter")
            if quality_cutoff:
                _ingest_check(_abi.set_quality(<ss_ingest*><size_t>g, quality_cutoff, quality_base), "ingest set quality")
            if _abi.fq_stages != NULL:
                _abi.fq_stages(<ss_ingest*><size_t>g, st_ms, &st_bytes)     # (drop what earlier calls left)
            jobs.append((g, 1, 0, 0, 0, fname, begin[k], begin[k + 1], line0[k], chunk_bytes, None))
        per = _run_shard_jobs(jobs)
        nseqs = sum(per)
        t2 = time.time()
        if _abi.fq_stages != NULL:    # the engines' stage split (before the reduce adds its finish)
            for d, g in engines:
                _abi.fq_stages(<ss_ingest*><size_t>g, st_ms, &st_bytes)
                stages.append([st_ms[i] for i in range(5)] + [st_bytes])
        counts = ShortSeqCounter()
        _reduce_fill(counts, engines, [sum(per[:k]) for k in range(D)])
        t3 = time.time()
        _last_fastq_stages[:] = [dict(zip(("read_ms", "h2d_dev_ms", "index_ms", "count_ms", "finish_ms", "h2d_bytes"), x))
                                 for x in stages]
        if _last_fastq_stages:
            _last_fastq_stages[0]["reduce_and_dict_ms"] = (t3 - t2) * 1e3
            _last_fastq_stages[0]["total_ms"] = (t3 - t1) * 1e3
    finally:
        free(begin)
        free(line0)
        for d, h in engines:
            _engine_nkeys.pop(h, None)
            if adapter is not None:      # (also on an engine that was counted again after SS_EFULL)
                _abi.set_adapter(<ss_ingest*><size_t>h, NULL, 0, 0, 0)
            if quality_cutoff:
                _abi.set_quality(<ss_ingest*><size_t>h, 0, 33)
            _engine_release(d, <ss_ingest*><size_t>h)
    print(f"{t2-t1:.2f}s to read {nseqs} total seqs, and {t3 - t2:.2f}s to count {len(counts)} unique sequences")
    return counts
