// The per-element terms of SAM's mask losses (maskloss.hip on stored full-resolution logits, samtail.hip on logits interpolated in
// registers): focal = af (1 - pt)^gamma bce, and d loss / d logit = c0 dfocal/dx + (c1 t + c2) p (1 - p).
#pragma once
#include "common.h"

struct MaskTerm {
    float p, bce, one_m_pt, af;
};

DEVINL MaskTerm mask_term(float x, float t, float alpha) {
    MaskTerm r;
    const float e = expf(-fabsf(x));
    r.p = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    r.bce = fmaxf(x, 0.f) - x * t + log1pf(e);
    r.one_m_pt = 1.f - (r.p * t + (1.f - r.p) * (1.f - t));
    r.af = alpha * t + (1.f - alpha) * (1.f - t);
    return r;
}

DEVINL float pow_gamma(float v, float gamma) {
    return gamma == 2.f ? v * v : powf(fmaxf(v, 0.f), gamma);
}

// d loss / d logit of one element (samtail.hip calls it; mask_loss_grad_kernel writes the same operations out, see there)
DEVINL float mask_term_grad(float x, float t, float alpha, float gamma, float c0, float c1, float c2) {
    const MaskTerm m = mask_term(x, t, alpha);
    const float sp = m.p * (1.f - m.p);
    const float dpt = sp * (2.f * t - 1.f);
    const float w_g = pow_gamma(m.one_m_pt, gamma);
    const float w_gm1 = gamma == 2.f ? m.one_m_pt : powf(fmaxf(m.one_m_pt, 0.f), gamma - 1.f);
    const float dfocal = m.af * (gamma * w_gm1 * (-dpt) * m.bce + w_g * (m.p - t));
    return c0 * dfocal + (c1 * t + c2) * sp;
}
