// El::Permutation / El::DistPermutation (include/El/core/Permutation.hpp,
// DistPermutation.hpp) as a swap sequence: applying it means swapping rows k and
// dest[k] for k = 0, 1, ... (the LAPACK ipiv, 0-based).  The sequence lives where
// the matrices it came from live: host memory for Device::CPU, device memory for
// Device::GPU, where LU's kernels write it and the row-permutation kernels read
// it, so it never has to cross to the host; a host copy is made only when asked
// for (SwapDests / ExplicitVector / Parity, which synchronise the stream).
// One class serves both names: the local and the distributed form differ only in
// the matrix PermuteRows is given.
#pragma once
#include "distmatrix.hpp"
#include <vector>

namespace elx {

class Permutation {
public:
    Permutation() = default;
    Permutation(const Permutation&) = delete;
    Permutation& operator=(const Permutation&) = delete;

    // the identity on n rows, no swaps, in the memory space of `dev`
    void MakeIdentity(Int n, Device dev = Device::CPU, hipStream_t s = nullptr);
    Int Height() const { return height_; }
    Int NumSwaps() const { return nswaps_; }
    Device Dev() const { return dev_; }
    hipStream_t Stream() const { return stream_; }

    // room for `total` swaps (kept ones stay); the array, in Dev()'s memory space
    int* Reserve(Int total);
    const int* Swaps() const { return static_cast<const int*>(swaps_.data()); }
    // the first k entries of the array are valid swaps, written on stream s
    void SetNumSwaps(Int k, hipStream_t s);

    // B := P B / P^-1 B: the swaps in order / in the opposite order.  Bit-exact.  An
    // [MC,MR] matrix on any grid is permuted in place, in runs of at most
    // Blocksize() swaps; other distributions go through the read-write proxy.
    void PermuteRows(DistMatrix& B) const;
    void InversePermuteRows(DistMatrix& B) const;
    // the swaps k0..k1-1 alone, on an [MC,MR] B of Height() rows
    void PermuteRowsRange(DistMatrix& B, Int k0, Int k1, bool inverse = false) const;

    std::vector<int64_t> SwapDests() const;       // dest[k], k < NumSwaps()
    std::vector<int64_t> ExplicitVector() const;  // (P B)(i, :) = B(v[i], :)
    bool Parity() const;                          // true: an odd permutation

private:
    void Run(DistMatrix& B, Int k0, Int nbr, bool inverse) const;
    Device dev_ = Device::CPU;
    hipStream_t stream_ = nullptr;
    Int height_ = 0, nswaps_ = 0, cap_ = 0;
    Buffer swaps_;
};

using DistPermutation = Permutation;

}  // namespace elx
