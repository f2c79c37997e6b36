// knn.cpp — gnss_knn_standardize / gnss_knn_classify: the k-NN classifier over standardised feature
// rows (the definition is in include/gnss_mi355x.h, the arithmetic in knn.h). The argument and
// bound checks, the host path (knn.h's knn_query over the queries on up to 16 threads) and the
// device path: the uploads, the scratch, the launch of knn.hip and the outputs' download. Built
// with -ffp-contract=off: every operation rounds on its own.
#include <cstring>
#include <vector>

#include "host.h"
#include "knn.h"

using namespace gnss;
using namespace gnss::host;

static_assert(sizeof(KnnDev) <= 1024, "KnnDev goes to the kernels by value");

namespace {

constexpr int kHostBlock = 64;  // queries a host thread takes at a time

void host_classify(const gnss_knn_model& m, int k, const double* q, int64_t Q, gnss_knn_out* out)
{
    const int64_t blocks = (Q + kHostBlock - 1) / kHostBlock;
    parallel_for((int)blocks, [&](int b) {
        double d2[kKnnMaxK];
        int32_t idx[kKnnMaxK];
        const int64_t hi = std::min<int64_t>(Q, ((int64_t)b + 1) * kHostBlock);
        for (int64_t i = (int64_t)b * kHostBlock; i < hi; i++) {
            double* pd = out->nn_d2 ? out->nn_d2 + i * k : d2;
            int32_t* pi = out->nn_index ? out->nn_index + i * k : idx;
            out->label[i] = knn_query(q + i * m.D, m.mu, m.inv, m.z, m.label, m.M, m.D, k, m.n_class, pd, pi,
                                      out->votes + i * m.n_class);
        }
    });
}

}  // namespace

extern "C" {

int gnss_knn_standardize(const double* x, int64_t M, int32_t D, double* mu, double* inv, double* z)
{
    if (!x || !mu || !inv || !z || M < 1 || M > kKnnMaxM || D < 1 || D > kKnnMaxD) return GNSS_EARG;
    for (int j = 0; j < D; j++)
        if (!knn_column_stats(x, M, D, j, mu + j, inv + j)) return GNSS_EARG;
    for (int64_t t = 0; t < M; t++)
        for (int j = 0; j < D; j++) z[t * D + j] = knn_z(x[t * D + j], mu[j], inv[j]);
    return GNSS_OK;
}

int gnss_knn_classify(gnss_ctx* ctx, const gnss_knn_cfg* cfg, const gnss_knn_model* model, const double* q, int64_t Q,
                      gnss_knn_out* out)
{
    if (!cfg || !model || !out) return fail(ctx, GNSS_EARG, "gnss_knn_classify: a null argument");
    const gnss_knn_model& m = *model;
    const int k = cfg->k;
    if (m.D < 1 || m.D > kKnnMaxD) return fail(ctx, GNSS_EARG, "gnss_knn_model.D outside 1..%d", kKnnMaxD);
    if (m.M < 1 || m.M > kKnnMaxM) return fail(ctx, GNSS_EARG, "gnss_knn_model.M outside 1..2^24");
    if (m.n_class < 1 || m.n_class > kKnnMaxClass)
        return fail(ctx, GNSS_EARG, "gnss_knn_model.n_class outside 1..%d", kKnnMaxClass);
    if (k < 1 || k > kKnnMaxK || k > m.M) return fail(ctx, GNSS_EARG, "gnss_knn_cfg.k outside 1..min(%d, M)", kKnnMaxK);
    if ((cfg->flags & ~GNSS_KNN_HOST) || (m.flags & ~GNSS_KNN_MODEL_DEVICE))
        return fail(ctx, GNSS_EARG, "gnss_knn_classify: an unknown flag");
    if (Q < 0 || Q > 0x7fffffff) return fail(ctx, GNSS_EARG, "gnss_knn_classify: Q outside 0..2^31-1");
    if (!m.mu || !m.inv || !m.z || !m.label) return fail(ctx, GNSS_EARG, "gnss_knn_model: a null array");
    if (!q || !out->label || !out->votes) return fail(ctx, GNSS_EARG, "gnss_knn_classify: a null array");
    const bool on_device = ctx && !(cfg->flags & GNSS_KNN_HOST);
    const bool dev_model = (m.flags & GNSS_KNN_MODEL_DEVICE) != 0;
    if (dev_model && !on_device) return fail(ctx, GNSS_EARG, "gnss_knn_classify: a device model needs the device path");
    if (on_device && !ctx->members.empty())
        return fail(ctx, GNSS_EARG, "gnss_knn_classify: the device path on a multi-device context");
    if (dev_model) {
        HIP_TRY(hipSetDevice(ctx->device));
        if (!device_memory_of(m.z, (size_t)m.M * m.D * sizeof(double), ctx->device) ||
            !device_memory_of(m.label, (size_t)m.M * sizeof(int32_t), ctx->device))
            return fail(ctx, GNSS_EARG, "gnss_knn_model: z / label are not M rows of device memory of the context's device");
    }

    // the training labels index the vote: a device model's come back for the check
    std::vector<int32_t> lab_copy;
    const int32_t* lab = m.label;
    if (dev_model) {
        HIP_TRY(hipSetDevice(ctx->device));
        lab_copy.resize((size_t)m.M);
        HIP_TRY(hipMemcpyAsync(lab_copy.data(), m.label, (size_t)m.M * sizeof(int32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        lab = lab_copy.data();
    }
    for (int64_t t = 0; t < m.M; t++)
        if (lab[t] < 0 || lab[t] >= m.n_class)
            return fail(ctx, GNSS_EARG, "gnss_knn_model.label[%lld] outside 0..n_class-1", (long long)t);
    if (Q == 0) return GNSS_OK;

    if (!on_device) {
        host_classify(m, k, q, Q, out);
        return GNSS_OK;
    }

    HIP_TRY(hipSetDevice(ctx->device));
    KnnDev d{};
    d.Q = Q;
    d.M = m.M;
    d.D = m.D;
    d.k = k;
    d.n_class = m.n_class;
    for (int j = 0; j < m.D; j++) {
        d.mu[j] = m.mu[j];
        d.inv[j] = m.inv[j];
    }
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    d.share = knn_split_share(m.M, Q, knn_block_slots(m.D, k, cus));
    d.splits = (int)((m.M + d.share - 1) / d.share);
    const size_t nq = (size_t)Q, nk = nq * (size_t)k, np = nk * (size_t)d.splits;
    DevBuf bq, bz, bl, pd, pt, ol, ov, oi, od;
    HIP_TRY(bq.alloc(ctx, "knn_q", nq * m.D * sizeof(double)));
    HIP_TRY(pd.alloc(ctx, "knn_part_d2", np * sizeof(double)));
    HIP_TRY(pt.alloc(ctx, "knn_part_t", np * sizeof(int32_t)));
    HIP_TRY(ol.alloc(ctx, "knn_label", nq * sizeof(int32_t)));
    HIP_TRY(ov.alloc(ctx, "knn_votes", nq * m.n_class * sizeof(int32_t)));
    HIP_TRY(oi.alloc(ctx, "knn_index", nk * sizeof(int32_t)));
    HIP_TRY(od.alloc(ctx, "knn_d2", nk * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(bq.p, q, nq * m.D * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (dev_model) {
        d.z = m.z;
        d.label = m.label;
    } else {
        HIP_TRY(bz.alloc(ctx, "knn_z", (size_t)m.M * m.D * sizeof(double)));
        HIP_TRY(bl.alloc(ctx, "knn_train_label", (size_t)m.M * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(bz.p, m.z, (size_t)m.M * m.D * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(bl.p, m.label, (size_t)m.M * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        d.z = bz.as<double>();
        d.label = bl.as<int32_t>();
    }
    d.q = bq.as<double>();
    d.part_d2 = pd.as<double>();
    d.part_t = pt.as<int32_t>();
    d.out_label = ol.as<int32_t>();
    d.out_votes = ov.as<int32_t>();
    d.out_index = oi.as<int32_t>();
    d.out_d2 = od.as<double>();
    const int le = knn_launch(d, ctx->stream);
    if (le) return fail(ctx, GNSS_EDEVICE, "gnss_knn_classify: kernel launch: %s", hipGetErrorString((hipError_t)le));
    HIP_TRY(hipMemcpyAsync(out->label, d.out_label, nq * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out->votes, d.out_votes, nq * m.n_class * sizeof(int32_t), hipMemcpyDeviceToHost,
                           ctx->stream));
    if (out->nn_index)
        HIP_TRY(hipMemcpyAsync(out->nn_index, d.out_index, nk * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out->nn_d2)
        HIP_TRY(hipMemcpyAsync(out->nn_d2, d.out_d2, nk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GNSS_OK;
}

}  // extern "C"
