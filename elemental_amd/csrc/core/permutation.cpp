// El::Permutation / El::DistPermutation: the swap sequence and its application
// to the rows of a distributed matrix.
#include "permutation.hpp"
#include "level3_internal.hpp"
#include "exec.hpp"
#include "../runtime/trace.hpp"
#include <algorithm>
#include <cstring>

namespace elx {

using namespace detail;

void Permutation::MakeIdentity(Int n, Device dev, hipStream_t s) {
    ELX_REQUIRE(n >= 0, "Permutation: negative height ", n);
    if (dev != dev_) {
        swaps_.Release();
        cap_ = 0;
    }
    dev_ = dev;
    hipStream_t ns = dev == Device::GPU ? (s ? s : Runtime::Get().ComputeStream()) : nullptr;
    if (dev == Device::GPU && cap_ > 0 && ns != stream_) {  // the kept array moves to the new stream
        StreamFence(stream_, ns);
        swaps_.Rebind(ns);
    }
    stream_ = ns;
    height_ = n;
    nswaps_ = 0;
    // a kept array starts over as zeros: nothing of an earlier permutation (of
    // another height, or of a factorization that failed) can be read as a swap
    if (cap_ > 0) {
        if (dev == Device::GPU) ELX_CHECK_HIP(hipMemsetAsync(swaps_.data(), 0, cap_ * sizeof(int), stream_));
        else std::memset(swaps_.data(), 0, cap_ * sizeof(int));
    }
}

int* Permutation::Reserve(Int total) {
    if (total > cap_) {
        // zero-filled, so entries a failed factorization never wrote are harmless swaps
        Buffer grown(dev_, static_cast<size_t>(total) * sizeof(int), stream_);
        if (dev_ == Device::GPU) {
            ELX_CHECK_HIP(hipMemsetAsync(grown.data(), 0, total * sizeof(int), stream_));
            if (nswaps_ > 0)
                ELX_CHECK_HIP(hipMemcpyAsync(grown.data(), swaps_.data(), nswaps_ * sizeof(int),
                                             hipMemcpyDeviceToDevice, stream_));
        } else {
            std::memset(grown.data(), 0, total * sizeof(int));
            if (nswaps_ > 0) std::memcpy(grown.data(), swaps_.data(), nswaps_ * sizeof(int));
        }
        swaps_ = std::move(grown);
        cap_ = total;
    }
    return static_cast<int*>(swaps_.data());
}

void Permutation::SetNumSwaps(Int k, hipStream_t s) {
    ELX_REQUIRE(k >= 0 && k <= cap_ && k <= height_, "Permutation: ", k, " swaps of ", height_, " rows");
    nswaps_ = k;
    if (dev_ == Device::GPU && s && s != stream_) {
        StreamFence(s, stream_);  // stream_ (where the array is freed and read back) follows the writer
    }
}

std::vector<int64_t> Permutation::SwapDests() const {
    std::vector<int> h(static_cast<size_t>(nswaps_));
    if (nswaps_ > 0) {
        if (dev_ == Device::GPU) {
            ELX_CHECK_HIP(hipMemcpyAsync(h.data(), swaps_.data(), nswaps_ * sizeof(int), hipMemcpyDeviceToHost,
                                         stream_));
            ELX_CHECK_HIP(hipStreamSynchronize(stream_));
        } else {
            std::memcpy(h.data(), swaps_.data(), nswaps_ * sizeof(int));
        }
    }
    return std::vector<int64_t>(h.begin(), h.end());
}

std::vector<int64_t> Permutation::ExplicitVector() const {
    const std::vector<int64_t> d = SwapDests();
    std::vector<int64_t> v(static_cast<size_t>(height_));
    for (Int i = 0; i < height_; ++i) v[i] = i;
    for (Int k = 0; k < nswaps_; ++k)
        if (d[k] >= 0 && d[k] < height_) std::swap(v[k], v[d[k]]);
    return v;
}

bool Permutation::Parity() const {
    const std::vector<int64_t> d = SwapDests();
    bool odd = false;
    for (Int k = 0; k < nswaps_; ++k) odd ^= d[k] != k;
    return odd;
}

namespace {

// the host forms of kern::perm_meta / perm_move / perm_apply (getrf.hip)
inline Int SlotRow(const int* piv, Int k0, Int nbr, Int q) { return q < nbr ? k0 + q : (Int)piv[k0 + q - nbr]; }

void HostMeta(const int* piv, Int k0, Int nbr, Int m, int stride, int align, int* meta) {
    for (Int q = 0; q < 2 * nbr; ++q) {
        const Int P = SlotRow(piv, k0, nbr, q);
        Int canon = q;
        if (P < 0 || P >= m) canon = -1;
        else if (q >= nbr) {
            if (P >= k0 && P < k0 + nbr) canon = P - k0;
            else
                for (Int t = nbr; t < q; ++t)
                    if ((Int)piv[k0 + t - nbr] == P) {
                        canon = t;
                        break;
                    }
        }
        meta[q] = (int)canon;
        meta[2 * nbr + q] = P < 0 ? 0 : (int)((P + align) % stride);
    }
}

template <typename U>
void HostMove(bool scatter, const int* piv, const int* meta, Int k0, Int nbr, int stride, int rank, U* A, Int lda,
              Int lw, U* buf) {
    const Int S = 2 * nbr;
    for (Int c = 0; c < lw; ++c)
        for (Int q = 0; q < S; ++q) {
            if (meta[q] != (int)q || meta[S + q] != rank) continue;
            const Int iloc = SlotRow(piv, k0, nbr, q) / stride;
            if (scatter) A[iloc + c * lda] = buf[q + c * S];
            else buf[q + c * S] = A[iloc + c * lda];
        }
}

template <typename U>
void HostApply(const int* meta, Int nbr, bool inverse, U* g, Int lw) {
    const Int S = 2 * nbr;
    for (Int t = 0; t < nbr; ++t) {
        const Int k = inverse ? nbr - 1 - t : t;
        const int a = meta[k], b = meta[nbr + k];
        if (a < 0 || b < 0 || a == b) continue;
        for (Int c = 0; c < lw; ++c)
            std::swap(g[((Int)meta[S + a] * lw + c) * S + a], g[((Int)meta[S + b] * lw + c) * S + b]);
    }
}

void CheckKern(hipError_t e, const char* what) {
    if (e != hipSuccess) throw HIPError(Cat(what, ": ", hipGetErrorName(e), " (", hipGetErrorString(e), ")"));
}

}  // namespace

// One run of swaps on an [MC,MR] matrix over r > 1 process rows.  Slot q < nbr
// stands for row k0 + q, slot nbr + q for row dest[k0 + q]: every process row packs
// the slots it owns into a 2 nbr x localWidth buffer, the buffers are all-gathered
// within the process column (as bytes: nothing is summed or converted, so -0 and
// NaN payloads survive), the swaps run on the gathered slots and the owners
// unpack.  The shapes depend on nbr and the grid only: the pivots stay where they are.
void Permutation::Run(DistMatrix& B, Int k0, Int nbr, bool inverse) const {
    const Grid& g = B.G();
    const int r = g.Height(), rank = g.MCRank(), align = B.ColAlign();
    const Int lw = B.LocalWidth(), S = 2 * nbr, ld = std::max<Int>(1, B.LDim());
    if (lw == 0 || nbr == 0) return;  // the whole process column has lw == 0
    const size_t es = B.ElemSize();
    const Device dev = B.Dev();
    hipStream_t s = B.Stream();
    Buffer meta(dev, static_cast<size_t>(2 * S) * sizeof(int), s), send(dev, static_cast<size_t>(S * lw) * es, s),
        recv(dev, static_cast<size_t>(r) * S * lw * es, s);
    int* mt = static_cast<int*>(meta.data());
    char* mine = static_cast<char*>(recv.data()) + static_cast<size_t>(rank) * S * lw * es;
    if (dev == Device::GPU) {
        CheckKern(kern::perm_meta(Swaps(), k0, nbr, height_, r, align, mt, s), "perm_meta");
        CheckKern(kern::perm_move(es, false, Swaps(), mt, k0, nbr, r, rank, B.Buffer(), ld, lw, send.data(), s),
                  "perm_move");
        g.MC().AllGather(DType::U8, send.data(), recv.data(), S * lw * (Int)es, dev, s);
        CheckKern(kern::perm_apply(es, mt, nbr, inverse, recv.data(), lw, s), "perm_apply");
        CheckKern(kern::perm_move(es, true, Swaps(), mt, k0, nbr, r, rank, B.Buffer(), ld, lw, mine, s), "perm_move");
        return;
    }
    HostMeta(Swaps(), k0, nbr, height_, r, align, mt);
    std::memset(send.data(), 0, send.bytes());
    if (es == 8) HostMove(false, Swaps(), mt, k0, nbr, r, rank, static_cast<uint64_t*>(B.Buffer()), ld, lw,
                          static_cast<uint64_t*>(send.data()));
    else HostMove(false, Swaps(), mt, k0, nbr, r, rank, static_cast<uint32_t*>(B.Buffer()), ld, lw,
                  static_cast<uint32_t*>(send.data()));
    g.MC().AllGather(DType::U8, send.data(), recv.data(), S * lw * (Int)es, dev, s);
    if (es == 8) {
        HostApply(mt, nbr, inverse, static_cast<uint64_t*>(recv.data()), lw);
        HostMove(true, Swaps(), mt, k0, nbr, r, rank, static_cast<uint64_t*>(B.Buffer()), ld, lw,
                 reinterpret_cast<uint64_t*>(mine));
    } else {
        HostApply(mt, nbr, inverse, static_cast<uint32_t*>(recv.data()), lw);
        HostMove(true, Swaps(), mt, k0, nbr, r, rank, static_cast<uint32_t*>(B.Buffer()), ld, lw,
                 reinterpret_cast<uint32_t*>(mine));
    }
}

void Permutation::PermuteRowsRange(DistMatrix& B, Int k0, Int k1, bool inverse) const {
    ELX_REQUIRE(B.ColDist() == Dist::MC && B.RowDist() == Dist::MR, "PermuteRows: not an [MC,MR] matrix");
    ELX_REQUIRE(0 <= k0 && k0 <= k1 && k1 <= nswaps_, "PermuteRows: swaps [", k0, ",", k1, ") of ", nswaps_);
    if (B.Height() != height_) throw LogicError("P and B must be the same height");
    RequireReal(B.Type(), "PermuteRows");
    if (B.Dev() != dev_) throw LogicError("PermuteRows: P and B live on different devices");
    if (k1 == k0 || B.Width() == 0) return;
    if (dev_ == Device::GPU) StreamFence(stream_, B.Stream());
    if (B.G().Height() == 1) {  // every row is local: the swaps themselves
        exec::Laswp(dev_, B.Type(), B.LocalHeight(), B.LocalWidth(), B.Buffer(), std::max<Int>(1, B.LDim()), Swaps(), k0,
                    k1, 0, inverse, nullptr, B.Stream());
    } else {
        const Int nb = std::max<Int>(1, Blocksize()), runs = (k1 - k0 + nb - 1) / nb;
        for (Int t = 0; t < runs; ++t) {
            const Int q = inverse ? runs - 1 - t : t, q0 = k0 + q * nb;
            Run(B, q0, std::min(nb, k1 - q0), inverse);
        }
    }
    // the array may be released or rewritten on stream_ once these reads are queued
    if (dev_ == Device::GPU) StreamFence(B.Stream(), stream_);
}

void Permutation::PermuteRows(DistMatrix& BPre) const {
    ELX_TRACE("El::Permutation::PermuteRows");
    if (BPre.Height() != height_) throw LogicError("P and B must be the same height");
    RWProxy Bp(BPre);
    PermuteRowsRange(Bp.Get(), 0, nswaps_, false);
    Bp.Finish();
}

void Permutation::InversePermuteRows(DistMatrix& BPre) const {
    ELX_TRACE("El::Permutation::InversePermuteRows");
    if (BPre.Height() != height_) throw LogicError("P and B must be the same height");
    RWProxy Bp(BPre);
    PermuteRowsRange(Bp.Get(), 0, nswaps_, true);
    Bp.Finish();
}

}  // namespace elx
