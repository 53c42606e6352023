// Stand-alone check of mdx_uniform_lj (molchanica_amd/csrc/mdx_hostutil.cpp): "does every atom with a Lennard-Jones well carry the same
// sigma / 2, and what is sigma_ij^2 then, as the pair kernel rounds it".  Built and run by tests/test_unilj_detect.py together with
// mdx_hostutil.cpp, with -fsanitize=address,undefined where the compiler has them; prints UNILJ-DETECT-OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

bool mdx_uniform_lj(const float* lj, size_t n, bool geometric, bool alch_on, float* c_out);

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the records mdx_create builds: (sigma / 2, sqrt(24 eps)) per atom
static std::vector<float> records(const std::vector<float>& sigma, const std::vector<float>& eps) {
    std::vector<float> r(2 * sigma.size());
    for (size_t i = 0; i < sigma.size(); ++i) { r[2 * i] = 0.5f * sigma[i]; r[2 * i + 1] = std::sqrt(24.0f * eps[i]); }
    return r;
}

int main() {
    const float so = 3.15061f, eo = 0.1521f;
    // what the device computes for two well-bearing atoms: fl(fl(h + h) * fl(h + h)), h = fl(sigma / 2)
    volatile float h = 0.5f * so; volatile float sum = h + h; volatile float want = sum * sum;
    float c = -1.f;

    {   // a water box: O, H, H with sigma_H = 0, eps_H = 0; N = 3 * 333 + 2 (no multiple of anything)
        std::vector<float> sg, ep;
        for (int i = 0; i < 1001; ++i) { const bool o = i % 3 == 0; sg.push_back(o ? so : 0.f); ep.push_back(o ? eo : 0.f); }
        const std::vector<float> r = records(sg, ep);
        CHECK(mdx_uniform_lj(r.data(), sg.size(), false, false, &c));
        CHECK(bits(c) == bits(want));
        // ... the same under the geometric rule or an alchemical window: refused, c = 0
        CHECK(!mdx_uniform_lj(r.data(), sg.size(), true, false, &c) && bits(c) == 0u);
        CHECK(!mdx_uniform_lj(r.data(), sg.size(), false, true, &c) && bits(c) == 0u);
        CHECK(mdx_uniform_lj(r.data(), sg.size(), false, false, nullptr));      // (no c wanted)
    }
    {   // all atoms equal, every one with a well
        const std::vector<float> r = records(std::vector<float>(17, so), std::vector<float>(17, eo));
        CHECK(mdx_uniform_lj(r.data(), 17, false, false, &c) && bits(c) == bits(want));
    }
    {   // atoms without a well carry foreign sigmas (hydrogens with a sigma, a dummy, an atom whose well was switched off): accepted
        const std::vector<float> r = records({1.0f, so, 0.4f, 7.5f, so, 0.f, 123.f}, {0.f, eo, 0.f, 0.f, 0.3f, 0.f, 0.f});
        CHECK(mdx_uniform_lj(r.data(), 7, false, false, &c) && bits(c) == bits(want));
    }
    {   // ... and the alchemical sign flag on a well-free atom (-0.0) is no well
        std::vector<float> r = records({1.0f, so, so}, {0.f, eo, eo});
        r[1] = -0.0f;
        CHECK(mdx_uniform_lj(r.data(), 3, false, false, &c) && bits(c) == bits(want));
    }
    {   // one well-bearing atom one ulp off, up or down, first or last: refused
        for (int where = 0; where < 2; ++where)
            for (int dir = 0; dir < 2; ++dir) {
                std::vector<float> r = records(std::vector<float>(9, so), std::vector<float>(9, eo));
                float& x = r[where ? 16 : 0];
                x = std::nextafterf(x, dir ? 10.f : 0.f);
                CHECK(!mdx_uniform_lj(r.data(), 9, false, false, &c) && bits(c) == 0u);
            }
        // ... the same atom without a well: accepted again
        std::vector<float> r = records(std::vector<float>(9, so), std::vector<float>(9, eo));
        r[16] = std::nextafterf(r[16], 10.f); r[17] = 0.f;
        CHECK(mdx_uniform_lj(r.data(), 9, false, false, &c) && bits(c) == bits(want));
    }
    {   // two LJ types (a solvated solute): refused
        const std::vector<float> r = records({so, 0.f, 0.f, 3.4f}, {eo, 0.f, 0.f, 0.1f});
        CHECK(!mdx_uniform_lj(r.data(), 4, false, false, &c));
    }
    {   // no atom has a well: refused
        const std::vector<float> r = records({so, so, 1.f}, {0.f, 0.f, 0.f});
        CHECK(!mdx_uniform_lj(r.data(), 3, false, false, &c) && bits(c) == 0u);
    }
    {   // N = 1 with and without a well, N = 0, no array
        const std::vector<float> a = records({so}, {eo}), b = records({so}, {0.f});
        CHECK(mdx_uniform_lj(a.data(), 1, false, false, &c) && bits(c) == bits(want));
        CHECK(!mdx_uniform_lj(b.data(), 1, false, false, &c));
        CHECK(!mdx_uniform_lj(a.data(), 0, false, false, &c));
        CHECK(!mdx_uniform_lj(nullptr, 5, false, false, &c));
    }
    {   // OPC's sigma, an odd mantissa: c is the rounded product of the rounded sum
        const float s2 = 3.16655f;
        volatile float h2 = 0.5f * s2; volatile float t = h2 + h2; volatile float w2 = t * t;
        const std::vector<float> r = records({s2, 0.f, 0.f, 0.f, s2, 0.f, 0.f, 0.f}, {0.2128f, 0.f, 0.f, 0.f, 0.2128f, 0.f, 0.f, 0.f});
        CHECK(mdx_uniform_lj(r.data(), 8, false, false, &c) && bits(c) == bits(w2));
        CHECK(bits(c) == bits((float)((double)(float)t * (double)(float)t)));      // (the f64 product of two f32 rounds once to f32: the same value)
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("UNILJ-DETECT-OK\n");
    return 0;
}
