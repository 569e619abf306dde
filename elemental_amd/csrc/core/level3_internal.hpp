// What level3.cpp and cholesky.cpp share with the SUMMA drivers in gemm.cpp.
// Internal: not installed, not part of the C ABI (gemm.hpp is the public header).
#pragma once
#include "gemm.hpp"
#include "redist.hpp"
#include <initializer_list>

namespace elx {
namespace detail {

inline bool IsN(int o) { return o == ELX_NORMAL; }

void FenceStreams(hipStream_t from, hipStream_t to);

// MultiSync (include/hydrogen/MultiSync.hpp:33-78): on entry the master stream
// waits for the others' queued work; on exit the others wait for the master, so
// a caller that reuses A or B on its own stream, and every temporary released
// on those streams, is ordered after the reads issued here.
class MultiSync {
public:
    MultiSync(hipStream_t master, std::initializer_list<hipStream_t> others) : master_(master), others_(others) {
        for (hipStream_t o : others_) FenceStreams(o, master_);
    }
    ~MultiSync() {
        for (hipStream_t o : others_) {
            try { FenceStreams(master_, o); } catch (...) {}
        }
    }
    MultiSync(const MultiSync&) = delete;
    MultiSync& operator=(const MultiSync&) = delete;

private:
    hipStream_t master_;
    std::vector<hipStream_t> others_;
};

// DistMatrixReadProxy<T,T,cd,rd,ELEMENT,D> (include/El/core/Proxy.hpp:174-300):
// the operands are brought to the device of `tgt` (the matrix being written,
// as Gemm/NN.hpp:357-359 proxies A and B onto C's device) and every read is
// queued on tgt's stream.  A itself (as a view on that stream) when it already
// has dist (cd,rd), that device [and the requested alignment]; else a
// redistributed copy, moved across devices when needed.
std::shared_ptr<const DistMatrix> ReadProxy(const DistMatrix& A, const DistMatrix& tgt, Dist cd, Dist rd,
                                            int calign = -1, int ralign = -1);

// DistMatrixReadWriteProxy for C: work in [MC,MR]; copy back on Finish().
struct RWProxy {
    DistMatrix& orig;
    std::shared_ptr<DistMatrix> tmp;
    explicit RWProxy(DistMatrix& C) : orig(C) {
        if (C.ColDist() != Dist::MC || C.RowDist() != Dist::MR) {
            tmp = C.Like(Dist::MC, Dist::MR);
            Copy(C, *tmp);
        }
    }
    DistMatrix& Get() { return tmp ? *tmp : orig; }
    void Finish() { if (tmp) Copy(*tmp, orig); }
};

// C-stationary SUMMA (gemm.cpp).  uplo >= 0: only C's lower (ELX_LOWER) or
// upper (ELX_UPPER) triangle is updated, through TrrkLocal.
void SummaC(int oA, int oB, double alpha, const DistMatrix& APre, const DistMatrix& BPre, double beta,
            DistMatrix& CPre, int uplo = -1);

// LocalTrrk: C_loc += alpha op(a) op(b) on the lower / upper triangle (by global index) of C's local block
void TrrkLocal(bool lower, bool ta, bool tb, Int k, double alpha, const void* a, Int lda, const void* b, Int ldb,
               DistMatrix& C, hipStream_t s, Buffer& tmp);

// A diagonal block where a local kernel reads it whole: A11 itself when its
// local storage already IS the [*,*] layout (a 1x1 grid: no redistribution
// temporary), else `stage` after A11[*,*] <- A11[MC,MR] (level3.cpp)
DistMatrix& StageDiagonalBlock(DistMatrix& A11, DistMatrix& stage);

}  // namespace detail
}  // namespace elx
