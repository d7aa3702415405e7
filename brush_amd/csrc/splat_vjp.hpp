// splat_vjp.hpp — the per-splat parameter VJP, the backward twin of splat_math.hpp: GatherGrads + ProjectBackwards of
// one visible splat from its compact-order gradient sums.
//
// Replaces:
//   GatherGrads       crates/brush-render/src/shaders/gather_grads.wgsl:165-232
//   ProjectBackwards  crates/brush-render/src/shaders/project_backwards.wgsl:75-227
// Built without FMA contraction (pragma below and -ffp-contract=off): same expression trees as the forward projection.
#pragma once
#include "internal.hpp"
#include "splat_math.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

// project_backwards.wgsl:25-57; G(a,b) = WGSL v_R[a][b] = column a, row b.
__device__ __forceinline__ void quat_to_rotmat_vjp(const float q[4], const Mat3 &vR, float o[4]) {
#define G(a, b) (vR.m[b][a])
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    o[0] = 2.0f * ((x * (G(1, 2) - G(2, 1)) + y * (G(2, 0) - G(0, 2))) + z * (G(0, 1) - G(1, 0)));
    o[1] = 2.0f * (((-2.0f * x * (G(1, 1) + G(2, 2)) + y * (G(0, 1) + G(1, 0))) + z * (G(0, 2) + G(2, 0))) +
                   w * (G(1, 2) - G(2, 1)));
    o[2] = 2.0f * (((x * (G(0, 1) + G(1, 0)) - 2.0f * y * (G(0, 0) + G(2, 2))) + z * (G(1, 2) + G(2, 1))) +
                   w * (G(2, 0) - G(0, 2)));
    o[3] = 2.0f * (((x * (G(0, 2) + G(2, 0)) + y * (G(1, 2) + G(2, 1))) - 2.0f * z * (G(0, 0) + G(1, 1))) +
                   w * (G(0, 1) - G(1, 0)));
#undef G
}

// What splat_projection_vjp hands to the camera-pose gradient: with p = W mean + t and T = J W,
//   v_p   the gradient at p: through the pixel position and through J (a depth gradient v_z is the caller's to add);
//   J     rows 0..1 of the UNCLAMPED Jacobian (row 2 is zero);
//   v_T   rows 0..1 of the gradient at T (row 2 meets the zero row of J: it contributes nothing to J^T v_T).
struct PoseTerms {
    float v_p[3], J[2][3], v_T[2][3];
};

// project_backwards.wgsl:59-72
__device__ __forceinline__ void cov2d_to_conic_vjp(const float conic[3], const float v_conic[3], float o[3]) {
    const float X[2][2] = {{conic[0], conic[1]}, {conic[1], conic[2]}};
    const float Gm[2][2] = {{v_conic[0], v_conic[1] / 2.0f}, {v_conic[1] / 2.0f, v_conic[2]}};
    float XG[2][2], S[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) XG[i][j] = X[i][0] * Gm[0][j] + X[i][1] * Gm[1][j];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) S[i][j] = XG[i][0] * X[0][j] + XG[i][1] * X[1][j];
    o[0] = -S[0][0];
    o[1] = -(S[0][1] + S[1][0]);
    o[2] = -S[1][1];
}

// ProjectBackwards for one splat (project_backwards.wgsl:83-226): (v_xy, v_conic) -> v_mean, v_scale (log
// space), v_quat.  Shared by the single-view kernels, the per-view record kernel and nothing else.
// AA (BRUSH_AUX_ANTIALIASED): v_comp, the gradient of the opacity factor comp, also enters v_cov2d
// (project_backwards.wgsl:112-128, disabled in the reference), and *comp_out receives comp, recomputed by the
// forward's own function from the same calc_cov2d outputs.
// PoseOut (void for the parameter backward: nothing is kept): the camera-pose gradient (pose_grad.hip) asks for the
// links of the same chain that end at the view matrix, see PoseTerms.
template <bool AA = false, typename PoseOut = void>
__device__ __forceinline__ void splat_projection_vjp(
    const ViewParams &vp, const float mean[3], const float scale[3], const float quat[4], const float vxy[2],
    const float vconic[3], float o_mean[3], float o_scale[3], float o_quat[4], float v_comp = 0.0f,
    float *comp_out = nullptr, PoseOut *pose = nullptr) {
    const Mat3 W = view_rot(vp);
    float p_view[3];
    to_view(vp, mean, p_view);
    float vpj[3];
    {  // project_pix_vjp :19-23
        const float rw = 1.0f / (p_view[2] + 1e-6f);
        const float vp0 = vp.focal[0] * vxy[0], vp1 = vp.focal[1] * vxy[1];
        vpj[0] = vp0 * rw;
        vpj[1] = vp1 * rw;
        vpj[2] = -(vp0 * p_view[0] + vp1 * p_view[1]) * rw * rw;
    }
    float vm[3];
#pragma unroll
    for (int i = 0; i < 3; i++) vm[i] = W.m[0][i] * vpj[0] + W.m[1][i] * vpj[1] + W.m[2][i] * vpj[2];

    float cov2d[3], conic[3], v_cov2d[3], raw[3];
    calc_cov2d(vp, p_view, scale, quat, cov2d, AA ? raw : nullptr);
    cov_to_conic(cov2d, conic);
    cov2d_to_conic_vjp(conic, vconic, v_cov2d);
    if constexpr (AA) {
        // comp^2 = det(S) / det(S + 0.3 I): d comp^2 / d(S + 0.3 I) = (1 - comp^2) conic - 0.3 det(conic) I, the
        // off-diagonal counted twice (cov2d_to_conic_vjp's convention for c01)
        const float comp = cov_compensation(raw, cov2d);
        *comp_out = comp;
        if (comp > 0.0f) {
            const float inv_det = conic[0] * conic[2] - conic[1] * conic[1];
            const float one_minus_sqr_comp = 1.0f - comp * comp;
            const float v_sqr_comp = v_comp * 0.5f / (comp + 1e-6f);
            v_cov2d[0] = v_cov2d[0] + v_sqr_comp * (one_minus_sqr_comp * conic[0] - kCovBlur * inv_det);
            v_cov2d[1] = v_cov2d[1] + 2.0f * v_sqr_comp * (one_minus_sqr_comp * conic[1]);
            v_cov2d[2] = v_cov2d[2] + v_sqr_comp * (one_minus_sqr_comp * conic[2] - kCovBlur * inv_det);
        }
    }

    const float rz = 1.0f / p_view[2];
    const float rz2 = rz * rz;
    // J from the UNCLAMPED p_view (project_backwards.wgsl:134-138)
    Mat3 J;
    J.m[0][0] = vp.focal[0] * rz; J.m[0][1] = 0.0f; J.m[0][2] = (-vp.focal[0]) * p_view[0] * rz2;
    J.m[1][0] = 0.0f; J.m[1][1] = vp.focal[1] * rz; J.m[1][2] = (-vp.focal[1]) * p_view[1] * rz2;
    J.m[2][0] = 0.0f; J.m[2][1] = 0.0f; J.m[2][2] = 0.0f;
    const Mat3 R = quat_to_rotmat(quat);
    Mat3 S;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) S.m[i][j] = (i == j) ? scale[i] : 0.0f;
    const Mat3 M = mul(R, S);
    const Mat3 V = mul(M, transpose(M));
    Mat3 v_cov;
    v_cov.m[0][0] = v_cov2d[0]; v_cov.m[0][1] = 0.5f * v_cov2d[1]; v_cov.m[0][2] = 0.0f;
    v_cov.m[1][0] = 0.5f * v_cov2d[1]; v_cov.m[1][1] = v_cov2d[2]; v_cov.m[1][2] = 0.0f;
    v_cov.m[2][0] = 0.0f; v_cov.m[2][1] = 0.0f; v_cov.m[2][2] = 0.0f;
    const Mat3 T = mul(J, W);
    const Mat3 Tt = transpose(T);
    const Mat3 Vt = transpose(V);
    const Mat3 v_V = mul(mul(Tt, v_cov), T);
    const Mat3 v_T = add(mul(mul(v_cov, T), Vt), mul(mul(transpose(v_cov), T), V));

    const float c0 = v_V.m[0][0];
    const float c1 = v_V.m[1][0] + v_V.m[0][1];
    const float c2 = v_V.m[2][0] + v_V.m[0][2];
    const float c3 = v_V.m[1][1];
    const float c4 = v_V.m[2][1] + v_V.m[1][2];
    const float c5 = v_V.m[2][2];

    const Mat3 v_J = mul(v_T, transpose(W));
    const float rz3 = rz2 * rz;
    const float vJ02 = v_J.m[0][2], vJ12 = v_J.m[1][2], vJ00 = v_J.m[0][0], vJ11 = v_J.m[1][1];
    float v_t[3];
    v_t[0] = (-vp.focal[0]) * rz2 * vJ02;
    v_t[1] = (-vp.focal[1]) * rz2 * vJ12;
    v_t[2] = (((-vp.focal[0]) * rz2 * vJ00 + 2.0f * vp.focal[0] * p_view[0] * rz3 * vJ02) -
              vp.focal[1] * rz2 * vJ11) +
             2.0f * vp.focal[1] * p_view[1] * rz3 * vJ12;
#pragma unroll
    for (int i = 0; i < 3; i++)
        o_mean[i] = vm[i] + ((v_t[0] * W.m[0][i] + v_t[1] * W.m[1][i]) + v_t[2] * W.m[2][i]);
    if constexpr (!std::is_void<PoseOut>::value) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            pose->v_p[i] = vpj[i] + v_t[i];
            pose->J[0][i] = J.m[0][i], pose->J[1][i] = J.m[1][i];
            pose->v_T[0][i] = v_T.m[0][i], pose->v_T[1][i] = v_T.m[1][i];
        }
    }

    Mat3 two_vVs;
    two_vVs.m[0][0] = 2.0f * c0; two_vVs.m[0][1] = 2.0f * (0.5f * c1); two_vVs.m[0][2] = 2.0f * (0.5f * c2);
    two_vVs.m[1][0] = 2.0f * (0.5f * c1); two_vVs.m[1][1] = 2.0f * c3; two_vVs.m[1][2] = 2.0f * (0.5f * c4);
    two_vVs.m[2][0] = 2.0f * (0.5f * c2); two_vVs.m[2][1] = 2.0f * (0.5f * c4); two_vVs.m[2][2] = 2.0f * c5;
    const Mat3 v_M = mul(two_vVs, M);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float vs = (R.m[0][j] * v_M.m[0][j] + R.m[1][j] * v_M.m[1][j]) + R.m[2][j] * v_M.m[2][j];
        o_scale[j] = vs * scale[j];  // log-space (:219)
    }
    const Mat3 v_R = mul(v_M, S);
    quat_to_rotmat_vjp(quat, v_R, o_quat);
}

// What the VJP reads of splat `g`: mean, exp(log_scale), quaternion.  (The three means loads, then the three log_scales
// loads: interleaving them costs the 12-byte vector loads.)
__device__ __forceinline__ void load_splat(const float *means, const float *log_scales, const float *quats, uint32_t g,
                                           float mean[3], float scale[3], float quat[4]) {
    mean[0] = means[(size_t)g * 3], mean[1] = means[(size_t)g * 3 + 1], mean[2] = means[(size_t)g * 3 + 2];
    scale[0] = det_expf(log_scales[(size_t)g * 3]), scale[1] = det_expf(log_scales[(size_t)g * 3 + 1]);
    scale[2] = det_expf(log_scales[(size_t)g * 3 + 2]);
    const float4 q4 = reinterpret_cast<const float4 *>(quats)[g];
    quat[0] = q4.x, quat[1] = q4.y, quat[2] = q4.z, quat[3] = q4.w;
}

// GatherGrads + ProjectBackwards of one visible splat `g` from its compact-order sums (r0, r1, r2): the parameter
// gradients and the factors of its v_sh row (Y[k] * vcol).  Shared by the single-view kernels; same expression trees in
// all.  AA: the compositing gradient v_alpha is with respect to the record's opacity sigmoid(raw) * comp (brush_hip.h:
// BRUSH_AUX_ANTIALIASED).
template <int DEG, bool AA = false>
__device__ __forceinline__ void visible_splat_vjp(
    const ViewParams &vp, const float *means, const float *log_scales, const float *__restrict__ quats,
    const float *raw_opac, uint32_t g, const float4 r0, const float4 r1, const float4 r2, float o_mean[3], float o_scale[3],
    float o_quat[4], float &o_opac, float o_xy[2], float vcol[3], float *Y) {
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);
    const float vxy[2] = {r0.x, r0.y};
    const float vconic[3] = {r0.z, r0.w, r1.x};
    vcol[0] = r1.y;
    vcol[1] = r1.z;
    vcol[2] = r1.w;
    const float v_alpha_sum = r2.x;
    float mean[3], scale[3], quat[4];
    load_splat(means, log_scales, quats, g, mean, scale, quat);

    // ---- GatherGrads (gather_grads.wgsl:174-231)
    float dir[3];
    view_dir(vp, mean, dir);
    sh_basis<ncoef>(DEG, dir, Y);
    const float sg = det_sigmoid(raw_opac[g]);
    if constexpr (AA) {
        // v_raw = v_alpha comp sigmoid (1 - sigmoid); v_comp = v_alpha sigmoid goes into the projection VJP
        o_xy[0] = vxy[0];
        o_xy[1] = vxy[1];
        float comp;
        splat_projection_vjp<true>(vp, mean, scale, quat, vxy, vconic, o_mean, o_scale, o_quat, v_alpha_sum * sg, &comp);
        o_opac = (v_alpha_sum * comp) * (sg * (1.0f - sg));
        return;
    }
    o_opac = v_alpha_sum * (sg * (1.0f - sg));
    o_xy[0] = vxy[0];
    o_xy[1] = vxy[1];

    // ---- ProjectBackwards (project_backwards.wgsl:83-226)
    splat_projection_vjp(vp, mean, scale, quat, vxy, vconic, o_mean, o_scale, o_quat);
}

}  // namespace
}  // namespace brush
