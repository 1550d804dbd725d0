// What reinit_cell_probe.hip (GPU) and reinit_cell_host.cpp (CPU) share: the manifest and the raw arrays.
//
//   PROGRAM DIR
//
// reads DIR/manifest.txt -- one case set per line, `name kind n=<cases> inf=<value>` -- and the raw little-endian
// arrays DIR/<name>.<tag>.bin, and writes DIR/<name>.<tag>.out:
//   update2 / update3   P [n][TDIM][TDIM], dv [n][TDIM] (double), ok [n][TDIM] (uint8)  ->  U [n]
//   seed2 / seed3       X [n][NV][TDIM], f [n][NV] (double)                             ->  flag [n] (uint8), dist [n][NV]
// (dist of a cell that is no seed cell is left at -1).  Nothing is generated or checked here: both stay in Python.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace cellio
{
struct Case
{
  std::string dir, name, kind;
  std::map<std::string, std::string> kv;
  std::string str(const char* key) const
  {
    auto it = kv.find(key);
    if (it == kv.end()) throw std::runtime_error(std::string("manifest: missing ") + key);
    return it->second;
  }
  int64_t num(const char* key) const { return atoll(str(key).c_str()); }
  double real(const char* key) const { return strtod(str(key).c_str(), nullptr); }
  std::string path(const std::string& tag, const char* ext) const { return dir + "/" + name + "." + tag + ext; }
};

inline std::vector<Case> manifest(const std::string& dir)
{
  std::ifstream in(dir + "/manifest.txt");
  if (!in) throw std::runtime_error("cannot open " + dir + "/manifest.txt");
  std::vector<Case> cases;
  std::string line;
  while (std::getline(in, line))
  {
    std::istringstream s(line);
    Case c;
    c.dir = dir;
    if (!(s >> c.name >> c.kind)) continue;
    std::string word;
    while (s >> word)
    {
      const size_t eq = word.find('=');
      if (eq == std::string::npos) throw std::runtime_error("manifest: not key=value: " + word);
      c.kv[word.substr(0, eq)] = word.substr(eq + 1);
    }
    cases.push_back(c);
  }
  return cases;
}

template <typename T>
std::vector<T> read_file(const std::string& path, int64_t n)
{
  std::vector<T> v((size_t)n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  const size_t got = n > 0 ? fread(v.data(), sizeof(T), (size_t)n, f) : 0;
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  if (got != (size_t)n || !at_end) throw std::runtime_error("wrong size: " + path);
  return v;
}

template <typename T>
void write_file(const std::string& path, const std::vector<T>& v)
{
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), f);
  if (fclose(f) != 0 || put != v.size()) throw std::runtime_error("short write: " + path);
}

inline int tdim_of(const Case& c)
{
  const char last = c.kind.empty() ? ' ' : c.kind.back();
  if ((c.kind != "update2" && c.kind != "update3" && c.kind != "seed2" && c.kind != "seed3")) throw std::runtime_error("unknown kind " + c.kind);
  return last - '0';
}
} // namespace cellio
