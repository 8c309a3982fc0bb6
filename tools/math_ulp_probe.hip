// Measures the ulp error of the device math functions the scoring path's row kernels lean on -- sqrtf, 1.0f / x, a / b, expf, logf -- as THIS build compiles them
// (the Makefile's flags), against the host's double precision, over argument files that tools/math_ulp_args.py writes from the row-kernel tests' own inputs.
// The figures stand in oracle/score_kernels_ref.py (ULP).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/math_ulp_probe.hip -o tools/bin/math_ulp_probe
//   python tools/math_ulp_args.py DIR && tools/bin/math_ulp_probe DIR [report.txt]
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__global__ void probe_kernel(int fn, const float* a, const float* b, float* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i];
    out[i] = fn == 0 ? sqrtf(x) : fn == 1 ? 1.0f / x : fn == 2 ? x / b[i] : fn == 3 ? expf(x) : logf(x);
}

static std::vector<float> read_floats(const std::string& path) {
    std::vector<float> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(bytes / 4);
    if (fread(v.data(), 4, v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s DIR [report]\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    FILE* rep = argc > 2 ? fopen(argv[2], "w") : nullptr;
    const char* names[5] = {"sqrt", "rcp", "div", "exp", "log"};
    for (int fn = 0; fn < 5; ++fn) {
        std::vector<float> a = read_floats(dir + "/" + names[fn] + ".bin"), b;
        if (fn == 2) b = read_floats(dir + "/div_b.bin");
        if (a.empty() || (fn == 2 && b.size() != a.size())) { fprintf(stderr, "%s: no arguments in %s\n", names[fn], dir.c_str()); return 2; }
        const long n = (long)a.size();
        float *da, *db = nullptr, *dout;
        CK(hipMalloc(&da, n * 4)); CK(hipMalloc(&dout, n * 4));
        CK(hipMemcpy(da, a.data(), n * 4, hipMemcpyHostToDevice));
        if (fn == 2) { CK(hipMalloc(&db, n * 4)); CK(hipMemcpy(db, b.data(), n * 4, hipMemcpyHostToDevice)); }
        hipLaunchKernelGGL(probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, da, db, dout, n);
        CK(hipGetLastError());
        std::vector<float> out(n);
        CK(hipMemcpy(out.data(), dout, n * 4, hipMemcpyDeviceToHost));
        double worst = 0.0, at = 0.0;
        long bad = 0, flushed = 0;
        for (long i = 0; i < n; ++i) {
            const double x = a[i];
            const double want = fn == 0 ? sqrt(x) : fn == 1 ? 1.0 / x : fn == 2 ? x / (double)b[i] : fn == 3 ? exp(x) : log(x);
            if (!std::isfinite(want) || !std::isfinite((double)out[i])) { bad += !(std::isfinite(want) == std::isfinite((double)out[i])); continue; }
            if (fabs(want) < ldexp(1.0, -126)) { flushed += (out[i] == 0.f && want != 0.0); continue; }        // denormal results: counted, not measured in ulps
            int ex;
            frexp(want, &ex);                                                                        // |want| in [2^(ex-1), 2^ex): ulp = 2^(ex - 24)
            const double err = fabs((double)out[i] - want) / ldexp(1.0, ex - 24);
            if (err > worst) { worst = err; at = x; }
        }
        char line[256];
        snprintf(line, sizeof line, "MATH_ULP fn=%s n=%ld worst_ulp=%.4f at=%.9g nonfinite_mismatch=%ld denormal_flushed=%ld\n", names[fn], n, worst, at, bad, flushed);
        fputs(line, stdout);
        if (rep) fputs(line, rep);
        CK(hipFree(da)); CK(hipFree(dout)); if (db) CK(hipFree(db));
    }
    if (rep) fclose(rep);
    return 0;
}
