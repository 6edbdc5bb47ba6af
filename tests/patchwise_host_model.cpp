// patchwise_host_model.cpp -- the __host__ __device__ grid / weight / blend functions of csrc/srx_patches.hpp run as a host loop
// (tests/test_patchwise_host.py builds this with g++ -fsanitize=address,undefined and compares the output with the numpy reference of
// tests/patchwise_cases.py bit for bit).
//   patchwise_host_model f32|f64 B H W PH PW SY SX MARGIN IN OUT
// IN: the patches [B P, PH, PW] as raw samples; OUT: the blended images [B, H, W].  The buffers are exactly as long as the shapes say:
// a read or a store outside them is the sanitizer's to report.  Prints: cy cx, then the origins of both axes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define SRX_PATCHES_HOST_ONLY
#include "srx_patches.hpp"

using namespace srx::patches;

template <typename T> static int run(int B, const BlendGeom &g, const char *in, const char *out)
{
    const size_t P = (size_t)g.cy * g.cx, n_in = (size_t)B * P * g.PH * g.PW, n_out = (size_t)B * g.H * g.W;
    std::vector<T> patches(n_in), img(n_out);
    FILE *fi = fopen(in, "rb");
    if (!fi || fread(patches.data(), sizeof(T), n_in, fi) != n_in || fgetc(fi) != EOF)
        return 2;
    fclose(fi);
    for (int b = 0; b < B; b++) {
        // a copy of exactly this image's patches: a read into a neighbour's is out of bounds here
        std::vector<T> item(patches.begin() + (size_t)b * P * g.PH * g.PW, patches.begin() + (size_t)(b + 1) * P * g.PH * g.PW);
        for (int y = 0; y < g.H; y++)
            for (int x = 0; x < g.W; x++)
                img[((size_t)b * g.H + y) * g.W + x] = blend_one<T>(item.data(), g, y, x);
    }
    FILE *fo = fopen(out, "wb");
    if (!fo || fwrite(img.data(), sizeof(T), n_out, fo) != n_out)
        return 2;
    fclose(fo);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 12) {
        fprintf(stderr, "usage: %s f32|f64 B H W PH PW SY SX MARGIN IN OUT\n", argv[0]);
        return 2;
    }
    const int B = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]), PH = atoi(argv[5]), PW = atoi(argv[6]), SY = atoi(argv[7]), SX = atoi(argv[8]),
              margin = atoi(argv[9]);
    const BlendGeom g{H, W, PH, PW, SY, SX, margin, grid_count(H, PH, SY), grid_count(W, PW, SX)};
    if (B <= 0 || g.cy == 0 || g.cx == 0 || margin < 0 || PH - SY - 2 * margin < 1 || PW - SX - 2 * margin < 1) {
        fprintf(stderr, "arguments no call accepts\n");
        return 2;
    }
    printf("%d %d", g.cy, g.cx);
    for (int i = 0; i < g.cy; i++)
        printf(" %d", grid_origin(i, H, PH, SY));
    for (int j = 0; j < g.cx; j++)
        printf(" %d", grid_origin(j, W, PW, SX));
    printf("\n");
    if (!strcmp(argv[1], "f32"))
        return run<float>(B, g, argv[10], argv[11]);
    if (!strcmp(argv[1], "f64"))
        return run<double>(B, g, argv[10], argv[11]);
    return 2;
}
