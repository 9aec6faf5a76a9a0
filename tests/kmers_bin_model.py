"""The .kmers.bin record format in numpy (src/io/IOUtils.java:39-65 printKmers, src/io/KmersLoadWorker.java:9-23): what
csrc/kmers_bin.hip's kernels must compute.  A record is the int64 key big-endian, then the int16 count big-endian."""
import numpy as np

RECORD = 10
HIST_BINS = 32768


def encode(keys, counts, threshold):
    """keys (int64) with their counts (int16, 0 .. 32767) in the order the records are wanted ->
    (the records with count > threshold as uint8 bytes, the histogram of ALL counts: 32768 bins of uint64)."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int16)
    assert len(keys) == len(counts) and (len(counts) == 0 or counts.min() >= 0)
    hist = np.bincount(counts.astype(np.int64), minlength=HIST_BINS).astype(np.uint64)
    sel = counts.astype(np.int64) > threshold
    out = np.zeros((int(sel.sum()), RECORD), dtype=np.uint8)
    out[:, :8] = keys[sel].astype(">i8").view(np.uint8).reshape(-1, 8)
    out[:, 8:] = counts[sel].astype(">i2").view(np.uint8).reshape(-1, 2)
    return out.reshape(-1), hist


def decode(data, freq_threshold):
    """bytes of whole records -> (keys int64, counts int16) of the records with count > freq_threshold (signed), in file order"""
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    assert len(raw) % RECORD == 0
    raw = raw.reshape(-1, RECORD)
    keys = raw[:, :8].copy().view(">i8").reshape(-1).astype(np.int64)
    counts = raw[:, 8:].copy().view(">i2").reshape(-1).astype(np.int16)
    sel = counts.astype(np.int64) > freq_threshold
    return keys[sel], counts[sel]


def stat_text(hist):
    """<name>.stat.txt of a histogram"""
    return "# k-mer frequency\tnumber of such k-mers\n" + "".join("%d\t%d\n" % (v, int(hist[v])) for v in np.nonzero(hist)[0]) + "\n"


def sorted_records(data):
    """the records of a file's bytes as (key, count) arrays sorted by key"""
    k, c = decode(data, -32769)
    o = np.argsort(k, kind="stable")
    return k[o], c[o]
