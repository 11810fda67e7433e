// Both forms of stage (4) of the rollout kernel — the loop over colliders and the (x, y)-pair form of the one-collider
// instantiations — compiled for the HOST from the kernel source itself and compared bit for bit on random poses
// (tests/test_contact_pairs_host.py cuts scal.inc and pair.inc out of csrc/mbd_kernels.h and stubs the device builtins).
#include "mbd_math.h"
#include <stdio.h>
#include <string.h>
#include <random>
using namespace mbd;
struct Inert { float inv_mass; float ib[1]; };
struct WI { float w[1]; };
static v3 crossz(v3 a) { return v3{a.y, -a.x, 0.0f}; }
static float dot_az0(v3 a, v3 b) { return ffma(a.x, b.x, a.y * b.y); }
static v3 cross_bz0(v3 a, v3 b) { return v3{-(a.z * b.y), a.z * b.x, ffma(a.x, b.y, -(a.y * b.x))}; }
template <bool ISO, bool AXI> static v3 iinv(const Inert& in, const WI&, v3 v) { return scale(v, in.ib[0]); }
template <bool ISO, bool AXI> static v3 iinv_z0(const Inert& in, const WI&, v3 v) { return v3{v.x * in.ib[0], v.y * in.ib[0], 0.0f}; }
struct Out { v3 cd_p, cd_th, pos; float dlam; bool act; };
struct In { v3 p, p_prev, col; q4 r, r_prev; float rad, mu, coll_scale; Inert ic; bool has; };
constexpr bool ISO = true, AXI = false;
static Out scalar_form(const In& I) {
  v3 p = I.p, p_prev = I.p_prev; q4 r = I.r, r_prev = I.r_prev; Inert ic = I.ic; WI Wc{{0}}; float mu = I.mu, coll_scale = I.coll_scale;
  v3 col_pos[1] = {I.col}; float col_rad[1] = {I.rad}; bool col_has[1] = {I.has};
  v3 cd_p = mk3(0, 0, 0), cd_th = mk3(0, 0, 0); v3 con_pos[1]; float con_dlam[1]; bool con_act[1];
  const int j = 0;
#include "scal.inc"
  return Out{cd_p, cd_th, con_pos[0], con_dlam[0], con_act[0]};
}
static Out pair_form(const In& I) {
  v3 p = I.p, p_prev = I.p_prev; q4 r = I.r, r_prev = I.r_prev; Inert ic = I.ic; float mu = I.mu, coll_scale = I.coll_scale;
  v3 col_pos[1] = {I.col}; float col_rad[1] = {I.rad}; bool col_has[1] = {I.has};
  v3 cd_p = mk3(0, 0, 0), cd_th = mk3(0, 0, 0); v3 con_pos[1]; float con_dlam[1]; bool con_act[1];
#include "pair.inc"
  return Out{cd_p, cd_th, con_pos[0], con_dlam[0], con_act[0]};
}
#ifndef N_CASES
#define N_CASES 400000
#endif
int main() {
  std::mt19937 g(1); std::normal_distribution<float> N(0, 1); std::uniform_real_distribution<float> U(0, 1);
  long bad = 0, n = 0, act = 0, stick = 0;
  for (long it = 0; it < N_CASES; ++it) {
    In I;
    float q[4] = {N(g), N(g), N(g), N(g)};
    int kind = it % 8;
    if (kind == 1) { q[1] = 0.0f; q[3] = -0.0f; }            // planar poses, zeros of either sign
    if (kind == 2) { q[1] = -0.0f; q[2] = 0.0f; }
    if (kind == 3) { q[0] = 1; q[1] = q[2] = q[3] = 0.0f; }
    if (kind == 4) { q[0] = 1; q[1] = -0.0f; q[2] = -0.0f; q[3] = -0.0f; }
    float nn = sqrtf(q[0]*q[0]+q[1]*q[1]+q[2]*q[2]+q[3]*q[3]) * (1.0f + 0.01f * N(g));
    I.r = q4{q[0]/nn, q[1]/nn, q[2]/nn, q[3]/nn};
    float e = (it % 3 == 0) ? 0.0f : 0.02f;
    I.r_prev = q4{I.r.w + e*N(g), I.r.x + e*N(g), I.r.y + e*N(g), I.r.z + e*N(g)};
    I.col = (it % 5 == 0) ? v3{0.1f*N(g), 0.1f*N(g), 0.1f*N(g)} : (it % 5 == 1 ? v3{0, 0, 0} : v3{0, 0, -0.12185684f});
    if (it % 10 == 6) I.col = v3{-0.0f, 0.0f, -0.12185684f};
    I.rad = 0.075f;
    v3 off = rot(I.col, I.r);
    float pen = (it % 4 == 0) ? 0.0f : (it % 4 == 1 ? 1e-3f * N(g) : 0.02f * U(g));
    I.p = v3{N(g), N(g), (I.rad - pen) - off.z};
    if (it % 16 == 2) I.p.z = 0.075f - off.z;  // exact touch where it rounds that way
    float sl = (it % 7 < 3) ? 1e-5f : 1e-2f;
    I.p_prev = (it % 6 == 0 && e == 0.0f) ? I.p : v3{I.p.x + sl*N(g), I.p.y + sl*N(g), I.p.z + sl*N(g)};
    I.mu = 1.0f; I.coll_scale = (it % 2) ? 1.0f : 0.5f; I.ic = Inert{0.3f + U(g), {2.0f + 10*U(g)}}; I.has = (it % 11) != 0;
    Out a = scalar_form(I), b = pair_form(I);
    n++; act += a.act; stick += a.act && (a.cd_p.x != 0 || a.cd_p.y != 0);
    bool same = memcmp(&a.cd_p, &b.cd_p, 12) == 0 && memcmp(&a.cd_th, &b.cd_th, 12) == 0 && a.act == b.act;
    // (the kernel reads the contact point and the multiplier only where the contact is active)
    if (a.act) same = same && memcmp(&a.pos, &b.pos, 12) == 0 && memcmp(&a.dlam, &b.dlam, 4) == 0;
    if (!same && bad++ < 5) printf("MISMATCH it=%ld act %d/%d cd_p %a %a %a | %a %a %a  cd_th %a %a %a | %a %a %a\n", it, a.act, b.act,
        a.cd_p.x, a.cd_p.y, a.cd_p.z, b.cd_p.x, b.cd_p.y, b.cd_p.z, a.cd_th.x, a.cd_th.y, a.cd_th.z, b.cd_th.x, b.cd_th.y, b.cd_th.z);
  }
  printf("%ld cases, %ld active, %ld with a tangential impulse, %ld mismatches\n", n, act, stick, bad);
  return bad != 0;
}
