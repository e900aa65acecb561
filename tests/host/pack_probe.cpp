// pack_probe — runs the engine's host-side weight packing (csrc/ag_pack.hip) on files, for tests/test_pack_host.py.  No GPU call.
//   pack_probe formats IN OUT   IN: floats.  OUT per value 8 bytes: u16 bf16_rne, u16 + u16 f16_split (hi, lo), u8 e4m3_rne, u8 0
//   pack_probe image IN OUT     IN: ag_model_config, then the 22 tensors in state_dict order (fp32, row-major).
//                               OUT: 12 u64 (off[2][4], off_h2, off_sc, h2_ok, image floats), then the image
#include "../../adaptigraph_amd/csrc/ag_pack.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ag_pack;

static std::vector<char> read_all(const char *path)
{
    std::vector<char> buf;
    FILE *f = fopen(path, "rb");
    if (!f) return buf;
    char chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    return buf;
}

static int write_all(const char *path, const std::vector<char> &buf)
{
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    return (fclose(f) == 0 && ok) ? 0 : 1;
}

template <class T> static void put(std::vector<char> &out, const T *p, size_t n)
{
    const char *c = reinterpret_cast<const char *>(p);
    out.insert(out.end(), c, c + n * sizeof(T));
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const std::vector<char> in = read_all(argv[2]);
    std::vector<char> out;
    if (!strcmp(argv[1], "formats")) {
        std::vector<float> v(in.size() / sizeof(float));
        memcpy(v.data(), in.data(), v.size() * sizeof(float));
        for (float x : v) {
            uint16_t w[3] = {bf16_rne(x), 0, 0};
            f16_split(x, w[1], w[2]);
            const uint8_t b[2] = {e4m3_rne(x), 0};
            put(out, w, 3);
            put(out, b, 2);
        }
    } else if (!strcmp(argv[1], "image")) {
        ag_model_config cfg;
        if (in.size() < sizeof cfg) return 3;
        memcpy(&cfg, in.data(), sizeof cfg);
        const size_t F = cfg.nf, dn = cfg.attr_dim + cfg.phys_dim + cfg.action_dim, de = 2 * cfg.attr_dim + 1 + 3 * cfg.n_his;
        const size_t count[N_TENSORS] = {F * dn, F, F * F, F, F * F, F, F * de, F, F * F, F, F * F, F, F * 2 * F, F, F * 3 * F, F,
                                         F * F, F, F * F, F, 3 * F, 3};
        std::vector<std::vector<float>> tensor(N_TENSORS);      // each its own allocation: a read past a tensor's end is an error, not a neighbour
        const float *ptr[N_TENSORS];
        size_t at = sizeof cfg;
        for (int i = 0; i < N_TENSORS; ++i) {
            if (at + count[i] * sizeof(float) > in.size()) return 3;
            tensor[i].resize(count[i]);
            memcpy(tensor[i].data(), in.data() + at, count[i] * sizeof(float));
            ptr[i] = tensor[i].data();
            at += count[i] * sizeof(float);
        }
        if (at != in.size()) return 3;
        const AgPackedWeights p = ag_pack_weights(cfg, ptr);
        const uint64_t head[12] = {p.off[0][0], p.off[0][1], p.off[0][2], p.off[0][3], p.off[1][0], p.off[1][1], p.off[1][2], p.off[1][3],
                                   p.off_h2, p.off_sc, p.h2_ok ? 1u : 0u, p.image.size()};
        put(out, head, 12);
        put(out, p.image.data(), p.image.size());
    } else {
        return 2;
    }
    return write_all(argv[3], out);
}
