// png_stream_fuzz.cpp — the host half of the stream PNG decoder (csrc/rtn_png_stream.h: the inspector and the CPU twin of the
// device's find, count, chain, marker decode, window walk and resolve; csrc/rtn_png_inflate.h) as a stand-alone program for a
// sanitizer build.  PSHostCtx aborts on any write or read outside the range it was given, so a clean exit under
// -fsanitize=address,undefined means no position derived from file bytes left its bounds.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iretinanet-for-table-detection_amd/csrc \
//       tools/png_stream_fuzz.cpp -o /tmp/png_stream_fuzz && /tmp/png_stream_fuzz 2000 page1.png page2.png ...
//
// For every file: the inspector on the file, on every prefix length around each chunk boundary and on 50 random prefixes, with an
// exactly sized blob; the twin at segment sizes 256, 1024, 4096 and 2^20 (status 0 and equal bytes expected for a valid file);
// then N copies of the blob with 1 .. 3 deflate bytes changed or the deflate data cut short, at a random segment size: status 0 only
// with the valid file's bytes.  Prints the number of cases and the links the valid files' chains had; exit status 1 on a mismatch.
#include "rtn_png_stream.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s CASES file.png ...\n", argv[0]); return 2; }
    const int cases = atoi(argv[1]);
    static const uint32_t sizes[4] = {256, 1024, 4096, 1u << 20};
    long inspected = 0, twins = 0, mutated = 0, accepted = 0, links_total = 0;
    for (int a = 2; a < argc; ++a) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) { perror(argv[a]); return 2; }
        std::vector<uint8_t> file;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) file.insert(file.end(), buf, buf + n);
        fclose(fp);
        char why[200];
        rtn_png_info_t info;
        // prefixes: an exactly sized heap copy, so that a read past the prefix is a sanitizer error
        std::vector<size_t> cuts;
        for (size_t pos = 8; pos + 12 <= file.size();) {
            const uint32_t len = ps_be32(file.data() + pos);
            for (int d = -1; d <= 1; ++d) cuts.push_back(pos + d);
            cuts.push_back(pos + 8);
            if ((size_t)len > file.size() - pos - 12) break;
            pos += 12 + (size_t)len;
        }
        for (int i = 0; i < 50; ++i) cuts.push_back(rnd((uint32_t)file.size()));
        for (size_t cut : cuts) {
            if (cut >= file.size()) continue;
            std::vector<uint8_t> part(file.begin(), file.begin() + cut);
            std::vector<uint8_t> blob(128 + 2 * cut);
            if (ps_inspect(part.data(), cut, 1024, &info, blob.data(), blob.size(), why, sizeof(why)) == RTN_OK) {
                fprintf(stderr, "%s: a prefix of %zu bytes was accepted\n", argv[a], cut);
                return 1;
            }
            ++inspected;
        }
        if (ps_inspect(file.data(), file.size(), 1024, &info, nullptr, 0, why, sizeof(why)) != RTN_OK) {
            fprintf(stderr, "%s: %s\n", argv[a], why);
            return 1;
        }
        std::vector<uint8_t> blob((size_t)info.blob_bytes);
        if (ps_inspect(file.data(), file.size(), 1024, &info, blob.data(), blob.size(), why, sizeof(why)) != RTN_OK) return 1;
        const size_t want = (size_t)info.height * (1 + (size_t)info.width * info.components);
        std::vector<uint8_t> good(want), out(want);
        const char* msg = "";
        int32_t st = -1;
        for (int s = 0; s < 4; ++s) {
            uint32_t links = 0;
            if (ps_inflate_host(blob.data(), blob.size(), sizes[s], s ? out.data() : good.data(), want, &st, &msg, &links) != RTN_OK || st != 0 ||
                (s && out != good)) {
                fprintf(stderr, "%s: segment %u: status %d %s\n", argv[a], sizes[s], st, msg);
                return 1;
            }
            printf("%s: segment %u: %u links\n", argv[a], sizes[s], links);
            links_total += links;
            ++twins;
        }
        PSHdr hd;
        memcpy(&hd, blob.data(), sizeof(hd));
        for (int i = 0; i < cases; ++i) {
            std::vector<uint8_t> m(blob);
            PSHdr h2 = hd;
            if (i & 1) {
                h2.in_bytes = 1 + rnd(hd.in_bytes);
                h2.nsegs = (h2.in_bytes + h2.seg_bytes - 1) / h2.seg_bytes;
                memcpy(m.data(), &h2, sizeof(h2));
            } else {
                for (uint32_t k = 1 + rnd(3); k > 0; --k) m[hd.off_data + rnd(hd.in_bytes)] ^= (uint8_t)(1 + rnd(255));
            }
            std::fill(out.begin(), out.end(), 0xa5);
            if (ps_inflate_host(m.data(), m.size(), sizes[rnd(4)], out.data(), want, &st, &msg) != RTN_OK) {
                fprintf(stderr, "%s: case %d: %s\n", argv[a], i, msg);
                return 1;
            }
            if (st == 0) {
                ++accepted;
                if (out != good) { fprintf(stderr, "%s: case %d: status 0 with other bytes\n", argv[a], i); return 1; }
            } else {
                for (uint8_t v : out)
                    if (v != 0xa5) { fprintf(stderr, "%s: case %d: status %d and out written\n", argv[a], i, st); return 1; }
            }
            ++mutated;
        }
    }
    printf("inspector prefixes %ld, valid twin runs %ld (%ld links), mutated or cut blobs %ld (%ld still valid)\n", inspected, twins,
           links_total, mutated, accepted);
    return 0;
}
