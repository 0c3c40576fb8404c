// Host-only run of the engine's blob parser and skeleton classifier (flygym_amd/csrc/nmf_skeleton.h) under the address and
// undefined-behaviour sanitizers.  No GPU and no HIP.  For every model blob named on the command line: the kernel family, the
// breadth-first tree tables and, for the hybrid families, the rest pack — or the refusal text.  tests/test_classify_check.py
// writes the blobs and checks what comes out.
//   c++ -std=c++17 -g -fsanitize=address,undefined -Iflygym_amd/csrc scripts/micro/classify_check.cpp -o classify_check
//   ./classify_check model.blob ...
#include <cstdio>
#include <fstream>
#include <iterator>

#include "nmf_skeleton.h"

static void print(const char* name, const std::vector<int>& v) {
  printf("  %s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::ifstream in(argv[a], std::ios::binary);
    const std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const char* base = strrchr(argv[a], '/');
    printf("%s\n", base ? base + 1 : argv[a]);
    std::string err;
    nmf_model* m = parse_model(bytes.data(), bytes.size(), err);
    if (!m) { printf("  refused %s\n", err.c_str()); continue; }
    Skeleton sk;
    if (const char* why = classify_skeleton(m, sk)) {
      printf("  refused %s\n", why);
    } else {
      printf("  family %d\n", sk.topo);
      print("lvl_start", sk.lvl_start); print("tree_body", sk.tree_body);
      print("child_start", sk.child_start); print("child_count", sk.child_count);
      if (nmf::family(sk.topo).hybrid()) {
        std::vector<int> pack;
        printf("  rest_fast %d\n", rest_pack_words(m, sk, pack) ? 1 : 0);
        print("rest_pack", pack);
      }
    }
    delete m;
  }
  return 0;
}
