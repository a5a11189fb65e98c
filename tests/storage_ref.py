"""Plain reference of everything a SparseStorage derives from its (row, col): numpy on the CPU.

Written from the definitions in paddle_sparse_amd/storage.py's docstrings, in the most obvious
way (np.bincount, np.cumsum, stable np.argsort, np.lexsort), so that every cache and private memo
an op hands over — sliced, shifted, swapped or concatenated from its operand's — can be compared
with what the result's own entries say it must be:

  rowptr / colptr     exclusive prefix sums of rowcount / colcount, M + 1 / N + 1 entries
  rowcount / colcount entries per row / column
  csr2csc             the STABLE permutation that orders the entries by column: csr2csc[j] is the
                      CSR position of the j-th entry in CSC order (equal columns stay in row order)
  csc2csr             its inverse: csc2csr[i] is the CSC position of CSR entry i
  row_csc / col_csc   row[csr2csc] / col[csr2csc]
  edge_tags(width)    position of every CSC-ordered entry inside its CSR row, in the row-local form
                      of csrc/vec_io.h: width 1 -> uint8, (index & 127) | 0x80 on rows of more than
                      128 entries; width 2 -> int16 holding index & 0xffff
  longest_row         max(rowcount), 0 without rows
  mean_scale          float32(1) / float32(max(rowcount, 1)) of the row of every entry, CSR order

Independent of the package and of oracle/storage_oracle.py: tests/test_storage_ref.py pins it to
hand-written matrices, to scipy.sparse and, once, to the oracle.
"""
from __future__ import annotations

import numpy as np

BYTE_EXACT_ROW = 128  # rows up to this many entries: the one-byte tag is the whole index (vec_io.h kByteExact)


class Derived:
    """Derived state of an M x N matrix with entries (row[i], col[i]), i in CSR (storage) order."""

    def __init__(self, row, col, M: int, N: int):
        row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
        assert row.ndim == 1 and row.shape == col.shape
        nnz = row.size
        if nnz:
            assert 0 <= row.min() and row.max() < M and 0 <= col.min() and col.max() < N, "index out of range"
        self.M, self.N, self.nnz = int(M), int(N), nnz
        self.row, self.col = row, col
        # row-major, non-decreasing (duplicates allowed): what every op must return
        self.sorted = bool(np.array_equal(np.lexsort((col, row)), np.arange(nnz))) if nnz else True
        self.rowcount = np.bincount(row, minlength=M).astype(np.int64)[:M]
        self.colcount = np.bincount(col, minlength=N).astype(np.int64)[:N]
        self.rowptr = np.concatenate([[0], np.cumsum(self.rowcount)]).astype(np.int64)
        self.colptr = np.concatenate([[0], np.cumsum(self.colcount)]).astype(np.int64)
        self.csr2csc = np.argsort(col, kind="stable").astype(np.int64)
        self.csc2csr = np.empty(nnz, np.int64)
        self.csc2csr[self.csr2csc] = np.arange(nnz, dtype=np.int64)
        self.row_csc, self.col_csc = row[self.csr2csc], col[self.csr2csc]
        self.longest_row = int(self.rowcount.max()) if M > 0 else 0
        deg = np.maximum(self.rowcount, 1).astype(np.float32)
        self.mean_scale = (np.float32(1.0) / deg)[row].astype(np.float32)

    def edge_tags(self, width: int) -> np.ndarray:
        # meaningful for a sorted storage only: entry i of row r sits at i - rowptr[r] inside it
        local = self.csr2csc - self.rowptr[self.row_csc]
        if width == 2:
            return (local & 0xffff).astype(np.uint16).view(np.int16)
        assert width == 1
        long_row = self.rowcount[self.row_csc] > BYTE_EXACT_ROW
        return ((local & 127) | np.where(long_row, 0x80, 0)).astype(np.uint8)


def derived(row, col, M: int, N: int) -> Derived:
    return Derived(row, col, M, N)
